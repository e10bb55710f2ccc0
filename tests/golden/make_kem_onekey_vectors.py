"""Writes tests/golden/kem_onekey_v1.json: what the reference's Kyber KEM (kyber/kem.c, compiled into oracle/_ref/libkyber_ref_k*.so by
oracle/Makefile) returns when ONE key serves many items -- the fixture of the one-key calls (kosk_kem_key_set, kosk_kem_enc_key,
kosk_kem_dec_key).  Only recorded results go into the file; the inputs are those of tests/kem_fixture.py.

    python tests/golden/make_kem_onekey_vectors.py

Per K in 2, 3, 4, with (pk, sk) = kf.keypair(K, 3):
  ct, ss     SHA3-256(ct) and ss of enc_derand(pk, kf.message(K, i)) for i = 0 .. 129, as two strings of 130 x 64 hex digits (items_of())
  dec        SHA3-256 over the 130 results of dec(ct_i, sk), back to back (each equals ss_i: asserted)
  ct5_hex    the ciphertext of item 5 in full
  tampered   dec(ct_5 with one bit flipped at byte b, sk) for b in kf.tamper_bytes(K)
  nc_pk      the pk re-encoded by kf.noncanonical_pk: [SHA3-256(ct), ss] of enc_derand(pk', m_i), i = 0 .. 7, and dec of those under
             sk' = s-hat || pk' || H(pk') || z (each equals ss: asserted)
  nc_shat    the s-hat of the sk re-encoded by kf.noncanonical_polyvec: dec(ct_i, sk'') for i = 0 .. 7 (the reference folds mod q: ss_i)
The generator asserts what it records: dec(ct) == ss for every canonical item, every rejection key == SHAKE256(z || ct) from hashlib,
and item 3 equals item 3 of kem_vectors_v1.json (the same key and message).
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import kem_fixture as kf  # noqa: E402
from tests.golden.make_kem_vectors import Ref  # noqa: E402

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kem_onekey_v1.json")
KEY, ITEMS, SHORT, TAMPER_ITEM = 3, 130, 8, 5


def items_of(v):
    """[[SHA3-256(ct) hex, ss hex]] of one K's canonical items"""
    return [[v["ct"][64 * i:64 * i + 64], v["ss"][64 * i:64 * i + 64]] for i in range(len(v["ss"]) // 64)]


def nc_pk_sk(k):
    """the key with its pk re-encoded: (pk', sk' = s-hat || pk' || H(pk') || z)"""
    pk, sk = kf.keypair(k, KEY)
    pk2, changed = kf.noncanonical_pk(pk, k)
    assert changed > 0
    return pk2, sk[:384 * k] + pk2 + hashlib.sha3_256(pk2).digest() + sk[-32:]


def nc_shat_sk(k):
    """the key with the s-hat of its sk re-encoded"""
    sk = kf.keypair(k, KEY)[1]
    body, changed = kf.noncanonical_polyvec(sk[:384 * k])
    assert changed > 0
    return body + sk[384 * k:]


def vectors(k):
    ref = Ref(k)
    pk, sk = kf.keypair(k, KEY)
    z = sk[-32:]
    items, decs, cts = [], [], []
    for i in range(ITEMS):
        ct, ss = ref.enc(pk, kf.message(k, i))
        d = ref.dec(ct, sk)
        assert d == ss, (k, i)
        items.append([kf.sha3(ct), ss.hex()])
        decs.append(d)
        cts.append(ct)
    old = kf.load()["k"]["k%d" % k][3]
    assert items[3] == [old["ct"], old["ss"]]
    out = {"ct": "".join(it[0] for it in items), "ss": "".join(it[1] for it in items), "dec": kf.sha3(b"".join(decs)),
           "ct5_hex": cts[TAMPER_ITEM].hex(), "tampered": []}
    for at in kf.tamper_bytes(k):
        bad = kf.tampered(cts[TAMPER_ITEM], at)
        d = ref.dec(bad, sk)
        assert d == hashlib.shake_256(z + bad).digest(32) and d != decs[TAMPER_ITEM]
        out["tampered"].append({"byte": at, "dec_ss": d.hex()})
    pk2, sk2 = nc_pk_sk(k)
    out["nc_pk"] = []
    for i in range(SHORT):
        ct, ss = ref.enc(pk2, kf.message(k, i))
        assert ct != cts[i] and ref.dec(ct, sk2) == ss
        assert ref.dec(ct, sk) == hashlib.shake_256(z + ct).digest(32)  # the canonical sk embeds another encoding: its rejection key
        out["nc_pk"].append([kf.sha3(ct), ss.hex()])
    sk3 = nc_shat_sk(k)
    out["nc_shat"] = [ref.dec(cts[i], sk3).hex() for i in range(SHORT)]
    assert out["nc_shat"] == [it[1] for it in items[:SHORT]]
    return out


def build():
    return {"format": "kosk-kem-onekey-v1", "key": KEY, "items": ITEMS, "k": {"k%d" % k: vectors(k) for k in (2, 3, 4)}}


def dump(obj):
    return json.dumps(obj, sort_keys=True, separators=(",", ":")).replace(',"', ',\n"') + "\n"


def main():
    text = dump(build())
    assert len(text) < 64 * 1024, len(text)
    with open(PATH, "w") as f:
        f.write(text)
    print(PATH, len(text), "bytes")


if __name__ == "__main__":
    main()
