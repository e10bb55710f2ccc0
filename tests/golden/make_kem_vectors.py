"""Writes tests/golden/kem_vectors_v1.json: what the reference's Kyber KEM (kyber/kem.c, compiled into oracle/_ref/libkyber_ref_k*.so
by oracle/Makefile) returns for the inputs defined in tests/kem_fixture.py.  Only recorded results go into the file.

    python tests/golden/make_kem_vectors.py

Per K in 2, 3, 4 and item i in 0 .. 129: SHA3-256 of pk, sk and ct, and ss, of enc_derand(pk_i, m_i); the full ct of items 0-3.
Key pairs come from this library's host key generation (api.host_keygen = kyber_keygen, kosk.cpp:4-70) and are pinned by their
digests: the reference's keypair_derand hashes its seed differently, and a test must be able to regenerate the keys without it.
(The KEM results therefore all come from the reference; only the keys differ from a keypair_derand fixture, and with them the number
of coefficients below 767 that item 2 re-encodes: 93 / 155 / 233 for K = 2 / 3 / 4, recorded as "noncanonical_coefficients", where keys
from keypair_derand on the same seeds would give 113 / 182 / 244.)
Item 2: encapsulation to the non-canonical encoding of its public key, and the reference's dec of that ciphertext under the canonical
secret key ("dec_ss": the rejection key, because the secret key embeds the canonical public key).
Item 3: the reference's dec of three single-bit tamperings of its ciphertext.
The generator checks what it records: dec(ct) == ss for every canonical item, and every rejection key == SHAKE256(z || ct).
"""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import kem_fixture as kf  # noqa: E402

NAMES = {2: "pqcrystals_kyber512_ref_", 3: "pqcrystals_kyber768_ref_", 4: "pqcrystals_kyber1024_ref_"}


class Ref:
    def __init__(self, k):
        self.k = k
        self.lib = C.CDLL(os.path.join(ROOT, "oracle", "_ref", "libkyber_ref_k%d.so" % k))
        self.enc_fn = getattr(self.lib, NAMES[k] + "enc_derand")
        self.dec_fn = getattr(self.lib, NAMES[k] + "dec")

    def enc(self, pk, m):
        ct = C.create_string_buffer(kf.CT_BYTES[self.k]); ss = C.create_string_buffer(32)
        self.enc_fn(ct, ss, C.c_char_p(pk), C.c_char_p(m))
        return ct.raw, ss.raw

    def dec(self, ct, sk):
        ss = C.create_string_buffer(32)
        self.dec_fn(ss, C.c_char_p(ct), C.c_char_p(sk))
        return ss.raw


def vectors(k):
    ref = Ref(k)
    items = []
    for i in range(kf.ITEMS):
        pk, sk = kf.keypair(k, i)
        assert sk[384 * k:384 * k + len(pk)] == pk and sk[-64:-32] == hashlib.sha3_256(pk).digest()
        z = sk[-32:]
        ct, ss = ref.enc(kf.enc_pk(k, i), kf.message(k, i))
        it = {"pk": kf.sha3(pk), "sk": kf.sha3(sk), "ct": kf.sha3(ct), "ss": ss.hex()}
        if i < 4:
            it["ct_hex"] = ct.hex()
        if i == 2:
            pk2, changed = kf.noncanonical_pk(pk, k)
            assert changed > 0 and ct != ref.enc(pk, kf.message(k, i))[0]
            it["noncanonical_coefficients"] = changed
            it["dec_ss"] = ref.dec(ct, sk).hex()
            assert it["dec_ss"] == hashlib.shake_256(z + ct).digest(32).hex()
        else:
            assert ref.dec(ct, sk) == ss
        if i == 3:
            it["tampered"] = []
            for at in kf.tamper_bytes(k):
                t = kf.tampered(ct, at)
                d = ref.dec(t, sk)
                assert d == hashlib.shake_256(z + t).digest(32)
                it["tampered"].append({"byte": at, "dec_ss": d.hex()})
        items.append(it)
    return items


def build():
    return {"format": "kosk-kem-v1", "items": kf.ITEMS, "k": {"k%d" % k: vectors(k) for k in (2, 3, 4)}}


def main():
    out = build()
    with open(kf.PATH, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(kf.PATH, os.path.getsize(kf.PATH), "bytes; non-canonical coefficients",
          [out["k"]["k%d" % k][2]["noncanonical_coefficients"] for k in (2, 3, 4)])


if __name__ == "__main__":
    main()
