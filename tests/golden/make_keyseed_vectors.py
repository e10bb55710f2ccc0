"""Writes tests/golden/keyseed_v1.json: seeds of format kosk-keyseed-v1 from the hashlib model tests/keyseed_model.py,
for K = 2, 3, 4, the keys of tests/golden/keyproof_keys_v1.json, context 00..1f, salt ff..e0 and the four flag combinations; each vector
holds the seed and the SHA3-256 of its kosk-seedtape-v1 tape.

    python tests/golden/make_keyseed_vectors.py
"""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import keyseed_model as km  # noqa: E402


def main():
    out = {"format": "kosk-keyseed-v1", "context": km.PIN_CONTEXT.hex(), "salt": km.PIN_SALT.hex(), "keys": "keyproof_keys_v1.json", "k": {}}
    for k in km.KS:
        nbytes, perms, last = km.shape(k)
        rows = []
        for i, sk in enumerate(km.fixture_keys(k)):
            for context, salt in km.flag_cases():
                s = km.seed(k, sk, context, salt)
                rows.append({"key": i, "flags": (1 if context is not None else 0) | (2 if salt is not None else 0), "seed": s.hex(),
                             "tape_sha3_256": hashlib.sha3_256(km.tape_from_seed(k, s)).hexdigest()})
        out["k"]["k%d" % k] = {"message_bytes": nbytes, "permutations": perms, "last_block_bytes": last, "vectors": rows}
    with open(km.FIXTURE, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", km.FIXTURE)


if __name__ == "__main__":
    main()
