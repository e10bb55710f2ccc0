"""Writes tests/golden/kem_edges_v1.json: what the reference's Kyber KEM (kyber/kem.c, compiled into oracle/_ref/libkyber_ref_k*.so by
oracle/Makefile) returns for the edge inputs defined in tests/kem_edges.py.  Only recorded results go into the file: digests, shared
secrets, block counts, integers -- and the ciphertexts of the four enc edges, so that a test can name the first differing byte.

    python tests/golden/make_kem_edge_vectors.py

Per K in 2, 3, 4:
  enc       enc_derand to the four one-value t-hat bodies: SHA3-256 of ct, ct, ss
  valid     CT = enc_derand(pk_H, m_H), the ciphertext most dec edges use: SHA3-256 of ct, ss
  dec       dec of every dec edge: the result, and whether it is the accept (== the ss of CT) or the rejection key; and m' =
            indcpa_dec of its ciphertext under its s-hat -- a rejection key does not depend on m', so decompress at every code and
            the fold of s-hat >= q are only visible there
  sampling  the searched keys a - d: per-entry SHAKE128 block counts and the candidate that became the 256th coefficient (from the
            restatement of rej_uniform in tests/kem_edges.py), SHA3-256 of ct and ss of enc_derand to the key; dec accepts
  four_block_items   which of the 130 items of kem_vectors_v1.json have an entry of A^T that needs a fourth block
  tamper_all         item 3's ciphertext with one bit flipped at every byte position: SHA3-256 over the concatenated dec results
The generator checks what it records: every rejection equals SHAKE256(z || ct) with the z stored in that sk, every accept equals the
ss of the encapsulation, the searched indices are what search() finds and meet their conditions, and every tampered ciphertext is
rejected.
"""
import ctypes as C
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from tests import kem_edges as ke  # noqa: E402
from tests import kem_fixture as kf  # noqa: E402
from make_kem_vectors import NAMES, Ref  # noqa: E402

ACCEPTS = ("shat_plus_q",)  # the dec edges the reference accepts


def indcpa_dec(ref, ct, sk):
    """indcpa_dec (kyber/indcpa.c:317-336) on the s-hat at the head of a KEM secret key"""
    m = C.create_string_buffer(32)
    getattr(ref.lib, NAMES[ref.k] + "indcpa_dec")(m, C.c_char_p(ct), C.c_char_p(sk[:384 * ref.k]))
    return m.raw


def rejection(sk, ct):
    return hashlib.shake_256(sk[-32:] + ct).digest(32)


def vectors(k):
    ref = Ref(k)
    out = {"enc": []}
    for name, pk, m in ke.enc_edges(k):
        ct, ss = ref.enc(pk, m)
        out["enc"].append({"name": name, "ct": kf.sha3(ct), "ct_hex": ct.hex(), "ss": ss.hex()})
    ct_valid, ss_valid = ref.enc(*ke.valid_input(k))
    assert ref.dec(ct_valid, kf.keypair(k, ke.HONEST)[1]) == ss_valid
    out["valid"] = {"ct": kf.sha3(ct_valid), "ss": ss_valid.hex()}
    out["plus_q_coefficients"] = kf.noncanonical_polyvec(kf.keypair(k, ke.HONEST)[1][:384 * k])[1]
    assert out["plus_q_coefficients"] > 0
    out["dec"] = []
    for name, ct, sk in ke.dec_edges(k, ct_valid):
        d = ref.dec(ct, sk)
        accept = d == ss_valid
        assert accept == (name in ACCEPTS), name
        assert accept or d == rejection(sk, ct), name
        mp = indcpa_dec(ref, ct, sk)
        assert not accept or mp == ke.valid_input(k)[1]
        out["dec"].append({"name": name, "accept": accept, "ss": d.hex(), "m": mp.hex()})
    out["sampling"] = []
    for cond, idx, m in ke.sampling_edges(k):
        assert idx == ke.search(k, cond), (k, cond)
        pk, sk = kf.keypair(k, idx)
        assert pk[-32:] == ke.rho_of_seed(k, kf.kg_seed(k, idx))
        stats = ke.matrix_stats(k, pk[-32:])
        assert ke.meets(cond, stats), (k, cond)
        ct, ss = ref.enc(pk, m)
        assert ref.dec(ct, sk) == ss
        out["sampling"].append({"cond": cond, "index": idx, "blocks": [s[0] for s in stats], "last": [s[1] for s in stats],
                                "ct": kf.sha3(ct), "ss": ss.hex()})
    out["four_block_items"] = [i for i in range(kf.ITEMS) if any(s[0] >= 4 for s in ke.matrix_stats(k, kf.keypair(k, i)[0][-32:]))]
    it = kf.load()["k"]["k%d" % k][ke.TAMPER_ITEM]
    ct3, sk3 = bytes.fromhex(it["ct_hex"]), kf.keypair(k, ke.TAMPER_ITEM)[1]
    assert ref.dec(ct3, sk3).hex() == it["ss"]
    h = hashlib.sha3_256()
    for t in ke.tamper_all(ct3):
        d = ref.dec(t, sk3)
        assert d == rejection(sk3, t) and d.hex() != it["ss"]
        h.update(d)
    out["tamper_all"] = {"item": ke.TAMPER_ITEM, "count": len(ct3), "digest": h.hexdigest()}
    return out


def build():
    return {"format": "kosk-kem-edges-v1", "k": {"k%d" % k: vectors(k) for k in (2, 3, 4)}}


def main():
    out = build()
    with open(ke.PATH, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(ke.PATH, os.path.getsize(ke.PATH), "bytes")
    for k in (2, 3, 4):
        v = out["k"]["k%d" % k]
        print("K=%d four-block entries among the %d items: %d items %s" % (k, kf.ITEMS, len(v["four_block_items"]), v["four_block_items"]))
        for s in v["sampling"]:
            print("K=%d (%s) key %d blocks %s last %s" % (k, s["cond"], s["index"], s["blocks"], s["last"]))


if __name__ == "__main__":
    main()
