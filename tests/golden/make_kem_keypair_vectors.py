"""Writes tests/golden/kem_keypair_v1.json: what the reference's crypto_kem_keypair_derand (kyber/kem.c:25-35, compiled into
oracle/_ref/libkyber_ref_k*.so by oracle/Makefile as pqcrystals_kyber{512,768,1024}_ref_keypair_derand) returns for the coins defined in
tests/kem_keypair_cases.py.  Only recorded results go into the file.

    python tests/golden/make_kem_keypair_vectors.py

Per K in 2, 3, 4 and item i in 0 .. 129: SHA3-256 of pk and of sk.  "four_block": the items whose matrix has an entry that needs a
fourth SHAKE128 block (about 6 % of all keys; the generator asserts that there is at least one per K).
The generator checks what it records: the sk embeds the pk, SHA3-256(pk) and z.
"""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import kem_keypair_cases as kk  # noqa: E402

NAMES = {2: "pqcrystals_kyber512_ref_", 3: "pqcrystals_kyber768_ref_", 4: "pqcrystals_kyber1024_ref_"}


def vectors(k):
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libkyber_ref_k%d.so" % k))
    fn = getattr(lib, NAMES[k] + "keypair_derand")
    pvb = 384 * k
    items, four = [], []
    for i in range(kk.ITEMS):
        c = kk.coins(k, i)
        pk, sk = C.create_string_buffer(pvb + 32), C.create_string_buffer(2 * pvb + 96)
        assert fn(pk, sk, C.c_char_p(c)) == 0
        pk, sk = pk.raw, sk.raw
        assert sk[pvb:2 * pvb + 32] == pk and sk[-64:-32] == hashlib.sha3_256(pk).digest() and sk[-32:] == c[32:]
        items.append({"pk": kk.sha3(pk), "sk": kk.sha3(sk)})
        if kk.needs_fourth_block(k, c):
            four.append(i)
    assert four, "K=%d: no item needs a fourth SHAKE128 block" % k
    return {"items": items, "four_block": four}


def build():
    return {"format": "kosk-keypair-v1", "items": kk.ITEMS, "k": {"k%d" % k: vectors(k) for k in kk.KS}}


if __name__ == "__main__":
    with open(kk.PATH, "w") as f:
        json.dump(build(), f, indent=1)
        f.write("\n")
    print("wrote", kk.PATH)
