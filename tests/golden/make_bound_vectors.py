"""Writes tests/golden/bound_v1.json: the pins of format kosk-bind-v1.

    python tests/golden/make_bound_vectors.py

The values come from hashlib and from the model that tests/bound_oracle.py derives from oracle/kosk_oracle.c -- NOT from the reference,
which has no such mode, and not from the library under test.  They pin the format across machines and compilers:
  bind    B for fixed (K, SHA3-256(pk), context) triples; the pk of triple i is SHAKE256("kosk-bind-v1:pk:<K>:<i>") cut to the key's length
  proofs  SHA3-256 of the bound proof for K = 2, 3, 4 on the tape SHAKE256("kosk-tape-v1:0") with the context 00 01 .. 1f
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

PK_BYTES = {2: 800, 3: 1184, 4: 1568}


def bind_cases():
    for k in (2, 3, 4):
        for i in range(3):
            pk = hashlib.shake_256(b"kosk-bind-v1:pk:%d:%d" % (k, i)).digest(PK_BYTES[k])
            ctx = [bytes(32), bytes(range(32)), hashlib.sha3_256(b"kosk-bind-v1:context:%d" % k).digest()][i]
            yield k, pk, ctx


def main():
    from tests import bound_oracle as bo
    out = {"format": "kosk-bind-v1", "bind": [], "proofs": {}}
    for k, pk, ctx in bind_cases():
        out["bind"].append({"K": k, "pk_sha3_256": hashlib.sha3_256(pk).hexdigest(), "context": ctx.hex(), "B": bo.bind_value(k, pk, ctx).hex()})
    for k in (2, 3, 4):
        pk, _, pi = bo.pinned(k)
        out["proofs"][str(k)] = {"pk_sha3_256": hashlib.sha3_256(pk).hexdigest(), "B": bo.bind_value(k, pk, bo.PIN_CONTEXT).hex(),
                                 "proof_sha3_256": hashlib.sha3_256(pi).hexdigest()}
    with open(os.path.join(HERE, "bound_v1.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


if __name__ == "__main__":
    main()
