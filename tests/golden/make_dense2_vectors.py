"""Writes tests/golden/dense_v2.json: the record sizes of the dense wire format kosk-dense-v2 for K = 2, 3, 4, computed from the format's
rule by tests/dense2_model.py (not read from the library), and the SHA-256 of the v2 record of the oracle's proof on tape 0
("kosk-tape-v1:0") per K, packed by the same model.

    python tests/golden/make_dense2_vectors.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import dense2_model as d2  # noqa: E402
from tests import oracle_lib  # noqa: E402


def main():
    out = {"format": "kosk-dense-v2", "tape": "kosk-tape-v1:0", "k": {}}
    for k in (2, 3, 4):
        pi = oracle_lib.verifiable_keygen(k, oracle_lib.tape_bytes_for(k, 0))[2]
        rc, rec = d2.pack(k, pi)
        assert rc == 0 and len(rec) == d2.dense2_bytes(k) and d2.unpack(k, rec) == (0, pi)
        out["k"][str(k)] = {"image_bytes": d2.image_bytes(k), "dense2_bytes": d2.dense2_bytes(k),
                            "record_sha256": hashlib.sha256(rec).hexdigest()}
    with open(os.path.join(HERE, "dense_v2.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
