"""Writes tests/golden/headsig_v1.json: vectors of format kosk-headsig-v1 under seed 00..1f and identifier 00..0f.
From the hashlib model tests/headsig_model.py: the public keys of heights 1, 2 and 5, the signatures at q = 0, 1 and 2^h - 1 (kyber_k 3,
roots headsig_cases.golden_root) and the cross-check values of the section.  From kosk_headsig_public_from_seed (Python is too slow
there; tests/test_headsig_host.py first proves the C function equal to the model up to height 5): the public keys of heights 10 and 11.
The two tags are the lowest for which the model sees a coefficient 0 and a coefficient 255 among the 32 signed heads of the signing
test and among the 15 items of the verifier's batch.

    python tests/golden/make_headsig_vectors.py
"""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tests import headsig_cases as hc  # noqa: E402
from tests import headsig_model as m  # noqa: E402


def lowest_tag(seen_of):
    tag = 0
    while not {0, 255} <= seen_of(tag):
        tag += 1
    return tag


def main():
    from mpcith_kyber_kosk_amd import api
    out = {"format": "kosk-headsig-v1", "seed": hc.SEED.hex(), "id": hc.ID.hex(), "kyber_k": hc.GOLDEN_K, "pub": {}, "sig": {}}
    for h in (1, 2, 5):
        key = hc.key(h)
        assert api.headsig_public_from_seed(h, hc.SEED, hc.ID) == key.pub
        out["pub"]["h%d" % h] = key.pub.hex()
        for q in sorted({0, 1, (1 << h) - 1}):
            sig = key.sign(hc.GOLDEN_K, hc.golden_root(h, q), q)
            assert m.verify(key.pub, hc.GOLDEN_K, hc.golden_root(h, q), q, sig)
            out["sig"]["h%d q%d" % (h, q)] = sig.hex()
    for h in (10, 11):
        out["pub"]["h%d" % h] = api.headsig_public_from_seed(h, hc.SEED, hc.ID).hex()
    root0 = bytes(32)
    S = m.statement(3, root0, 0)
    C0 = m.randomizer(hc.ID, 0, hc.SEED)
    out["cross_check"] = {"x_0[0]": m.x_start(hc.ID, 0, 0, hc.SEED).hex(), "C_0": C0.hex(), "T[1] h1": hc.key(1).T[1].hex(),
                          "T[1] h5": hc.key(5).T[1].hex(), "statement root 00^32 size 0 k 3": S.hex(), "Q of that statement under C_0": m.digest(hc.ID, 0, C0, S).hex()}
    out["sign_tag"] = lowest_tag(lambda t: hc.history_signatures(hc.K, t)[1])
    out["batch_tag"] = lowest_tag(lambda t: hc.batch_items(hc.K, t, 15)[3])
    sigs, _ = hc.history_signatures(hc.K, out["sign_tag"])
    out["history_signatures_sha3_256"] = hashlib.sha3_256(b"".join(sigs)).hexdigest()
    with open(hc.GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", hc.GOLDEN, "sign_tag", out["sign_tag"], "batch_tag", out["batch_tag"])


if __name__ == "__main__":
    main()
