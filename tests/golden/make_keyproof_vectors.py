"""Writes tests/golden/keyproof_keys_v1.json: two Kyber key pairs per K that this library never made -- what the reference's
crypto_kem_keypair_derand (kyber/kem.c:25-37, compiled into oracle/_ref/libkyber_ref_k*.so by oracle/Makefile) returns on the coins
SHAKE256("kosk-keyproof-v1:K:i", 64), i = 0, 1.  Only recorded results go into the file.

    python tests/golden/make_keyproof_vectors.py

The generator checks what it records: the pk inside the sk is the pk, and H(pk) follows it.
"""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import keyproof_cases as kc  # noqa: E402

NAMES = {2: "pqcrystals_kyber512_ref_", 3: "pqcrystals_kyber768_ref_", 4: "pqcrystals_kyber1024_ref_"}
PER_K = 2


def keypair(k, coins):
    lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libkyber_ref_k%d.so" % k))
    pk = C.create_string_buffer(384 * k + 32); sk = C.create_string_buffer(768 * k + 96)
    getattr(lib, NAMES[k] + "keypair_derand")(pk, sk, C.c_char_p(coins))
    return pk.raw, sk.raw


def build():
    out = {"format": "kosk-keyproof-v1", "per_k": PER_K, "k": {}}
    for k in kc.KS:
        items = []
        for i in range(PER_K):
            pk, sk = keypair(k, kc.foreign_coins(k, i))
            assert sk[384 * k:768 * k + 32] == pk and sk[768 * k + 32:768 * k + 64] == hashlib.sha3_256(pk).digest()
            items.append({"pk_sha3": hashlib.sha3_256(pk).hexdigest(), "sk": sk.hex()})  # the pk itself is sk[384 K : 768 K + 32]
        out["k"]["k%d" % k] = items
    return out


def main():
    out = build()
    with open(kc.FIXTURE, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(kc.FIXTURE, os.path.getsize(kc.FIXTURE), "bytes")


if __name__ == "__main__":
    main()
