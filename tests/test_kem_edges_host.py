"""Kyber KEM edge vectors, the part that needs no GPU: the fixture tests/golden/kem_edges_v1.json (its shape, the checks that need no
reference, the whole file again from oracle/_ref where that exists -- KOSK_REQUIRE_REF=1 makes its absence a failure), the sampling
conditions of the searched keys, and the device functions of csrc/kosk_kem_dev.hpp built for the host (tools/kem_host_model.cpp) on
every edge item and on a ciphertext tampered with at every byte.  If the model agrees with the reference here and a GPU test of
tests/test_gpu_16_kem_edges.py does not, the fault is in the kernels' work distribution or the host code, not in kosk_kem_dev.hpp."""
import ctypes as C
import hashlib
import os
import sys

import pytest

from tests import kem_edges as ke
from tests import kem_fixture as kf
from tests.test_kem_host import model  # noqa: F401  (the host build of the device functions, one per module)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (2, 3, 4)
DEC_NAMES = (["shat_%s:ct_%s" % (s, c) for s in ("fff", "zero", "qm1") for c in ("valid", "ff", "00", "random")]
             + ["honest:ct_ff", "honest:ct_00", "honest:ct_random", "honest:ct_codes_up", "honest:ct_codes_down", "shat_plus_q", "stored_h_flip", "foreign_pk_tail", "other_z:ct_tampered"])


def test_fixture_shape():
    fx = ke.load()
    assert fx["format"] == "kosk-kem-edges-v1" and sorted(fx["k"]) == ["k2", "k3", "k4"]
    for k in KS:
        v = fx["k"]["k%d" % k]
        assert [e["name"] for e in v["enc"]] == ["that_fff", "that_zero", "that_qm1", "that_q"]
        assert all(len(e["ct_hex"]) == 2 * kf.CT_BYTES[k] and len(e["ss"]) == 64 for e in v["enc"])
        assert [d["name"] for d in v["dec"]] == DEC_NAMES and len(DEC_NAMES) == 21
        assert [d["name"] for d in v["dec"] if d["accept"]] == ["shat_plus_q"]
        assert [(s["cond"], s["index"]) for s in v["sampling"]] == [(c, ke.SAMPLING[k][c]) for c in ke.CONDS]
        assert all(len(s["blocks"]) == k * k == len(s["last"]) for s in v["sampling"])
        assert v["tamper_all"]["item"] == ke.TAMPER_ITEM and v["tamper_all"]["count"] == kf.CT_BYTES[k]
    assert os.path.getsize(ke.PATH) < 1 << 17  # digests, not bytes: far below the 1 MiB bound on a committed file


def test_inputs_are_the_edges_they_claim_to_be():
    for k in KS:
        names = dict((n, pk) for n, pk, _ in ke.enc_edges(k))
        assert names["that_fff"][:384 * k] == b"\xff" * (384 * k) and names["that_zero"][:384 * k] == bytes(384 * k)
        assert names["that_qm1"][:384 * k] == bytes.fromhex("000dd0") * (128 * k) and names["that_q"][:384 * k] == bytes.fromhex("011dd0") * (128 * k)
        assert len(set(pk[-32:] for pk in names.values())) == 4
        assert all(len(pk) == 384 * k + 32 for pk in names.values())
        pk, sk = kf.keypair(k, ke.HONEST)
        body, changed = kf.noncanonical_polyvec(sk[:384 * k])
        assert changed == ke.load()["k"]["k%d" % k]["plus_q_coefficients"] > 0 and body != sk[:384 * k]
        assert kf.noncanonical_polyvec(body)[1] == 0  # nothing below 767 is left
        assert kf.noncanonical_pk(pk, k) == (kf.noncanonical_polyvec(pk[:384 * k])[0] + pk[-32:], kf.noncanonical_polyvec(pk[:384 * k])[1])
        ct = bytes(range(256)) * 7
        ts = ke.tamper_all(ct[:kf.CT_BYTES[k]])
        assert len(ts) == kf.CT_BYTES[k] and all(bytes(a ^ b for a, b in zip(t, ct)).strip(b"\0") == bytes([1 << (at % 8)])
                                                 and t[at] != ct[at] for at, t in enumerate(ts))


@pytest.mark.parametrize("k", KS)
def test_sampling_conditions(k):
    """the searched keys meet a - d, recomputed here from the regenerated keys with the restatement of rej_uniform; and the number of
    items of kem_vectors_v1.json with a four-block entry is what the fixture records (whatever it is)"""
    v = ke.load()["k"]["k%d" % k]
    for s in v["sampling"]:
        pk = kf.keypair(k, s["index"])[0]
        assert pk[-32:] == ke.rho_of_seed(k, kf.kg_seed(k, s["index"]))
        stats = ke.matrix_stats(k, pk[-32:])
        assert [t[0] for t in stats] == s["blocks"] and [t[1] for t in stats] == s["last"]
        assert ke.meets(s["cond"], stats), (k, s["cond"])
    by = {s["cond"]: s for s in v["sampling"]}
    assert 4 in by["a"]["blocks"] and max(by["a"]["blocks"]) == 4
    assert ke.LAST_OF_THIRD_BLOCK == 335 in by["b"]["last"]
    c_stats = ke.matrix_stats(k, kf.keypair(k, by["c"]["index"])[0][-32:])
    assert any(t[1] % 2 == 0 and t[2] for t in c_stats)
    assert by["d"]["blocks"] == [3] * (k * k)
    four = [i for i in range(kf.ITEMS) if any(t[0] >= 4 for t in ke.matrix_stats(k, kf.keypair(k, i)[0][-32:]))]
    assert four == v["four_block_items"]
    print("K=%d: %d of %d fixture items have a four-block entry: %s" % (k, len(four), kf.ITEMS, four))


def test_entry_stats_on_a_made_up_stream(monkeypatch):
    """the restatement itself: candidate order d1, d2 per group, the drop of a second half after the 256th coefficient, block counting"""
    class Fake:
        def __init__(self, stream):
            self.stream = stream

        def digest(self, n):
            return (self.stream + bytes(n))[:n]
    grp = lambda d1, d2: bytes([d1 & 0xFF, (d1 >> 8) | ((d2 & 0xF) << 4), d2 >> 4])
    cases = [(grp(1, 2) * 128, (3, 255, False)),                      # 256th = second half of group 127
             (grp(1, 0xFFF) * 255 + grp(5, 6), (5, 510, True)),       # first half, droppable second half; group 255 is in block 5
             (grp(1, 0xFFF) * 255 + grp(5, ke.Q), (5, 510, False)),
             (grp(ke.Q, 0xD00) * 256, (5, 511, False)),               # q itself is rejected, q - 1 accepted
             (grp(1, 2) * 111 + grp(0xFFF, 0xFFF) * 56 + grp(0xFFF, 0xFFF) + grp(3, 4) * 17, (4, 2 * 184 + 1, False))]
    for stream, want in cases:
        monkeypatch.setattr(ke.hashlib, "shake_128", lambda data, s=stream: Fake(s))
        assert ke.entry_stats(bytes(32), 0, 0) == want


@pytest.mark.parametrize("k", KS)
def test_fixture_internal_checks(k, model):  # noqa: F811
    """without the reference: every recorded rejection is SHAKE256(z || ct) with the z of the sk the item was given, every accept is
    the recorded ss of the valid ciphertext, and the stored ciphertexts hash to the stored digests (the valid ciphertext comes from
    the host model, checked against its recorded digest first)"""
    v = ke.load()["k"]["k%d" % k]
    for e in v["enc"]:
        assert kf.sha3(bytes.fromhex(e["ct_hex"])) == e["ct"]
    ct_valid = _model_enc(model, k, *ke.valid_input(k))[0]
    assert kf.sha3(ct_valid) == v["valid"]["ct"]
    for (name, ct, sk), d in zip(ke.dec_edges(k, ct_valid), v["dec"]):
        assert name == d["name"]
        assert d["ss"] == (v["valid"]["ss"] if d["accept"] else hashlib.shake_256(sk[-32:] + ct).digest(32).hex()), name
    it =kf.load()["k"]["k%d" % k][ke.TAMPER_ITEM]
    sk3 = kf.keypair(k, ke.TAMPER_ITEM)[1]
    h = hashlib.sha3_256()
    for t in ke.tamper_all(bytes.fromhex(it["ct_hex"])):
        h.update(hashlib.shake_256(sk3[-32:] + t).digest(32))
    assert h.hexdigest() == v["tamper_all"]["digest"]


def test_fixture_equals_reference():
    """the whole file again from oracle/_ref/libkyber_ref_k*.so (the generator asserts what it records on the way)"""
    missing = [p for p in (os.path.join(ROOT, "oracle", "_ref", "libkyber_ref_k%d.so" % k) for k in KS) if not os.path.exists(p)]
    if missing:
        if os.environ.get("KOSK_REQUIRE_REF") == "1":
            pytest.fail("KOSK_REQUIRE_REF=1 but %s is missing: run `make -C oracle` where the reference tree is mounted" % missing[0])
        return  # the internal checks above are what runs here
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_kem_edge_vectors
    finally:
        sys.path.pop(0)
    assert make_kem_edge_vectors.build() == ke.load()


def _model_enc(model, k, pk, m):  # noqa: F811
    ct, ss = C.create_string_buffer(kf.CT_BYTES[k]), C.create_string_buffer(32)
    assert model.kem_model_enc(k, pk, m, ct, ss) == 0
    return ct.raw, ss.raw


def _model_dec(model, k, ct, sk):  # noqa: F811
    ss = C.create_string_buffer(32)
    assert model.kem_model_dec(k, ct, sk, ss) == 0
    return ss.raw


@pytest.mark.parametrize("k", KS)
def test_device_functions_on_the_host_match_the_edge_fixture(model, k):  # noqa: F811
    v = ke.load()["k"]["k%d" % k]
    for (name, pk, m), e in zip(ke.enc_edges(k), v["enc"]):
        ct, ss = _model_enc(model, k, pk, m)
        if ct.hex() != e["ct_hex"]:
            want = bytes.fromhex(e["ct_hex"])
            at = next(j for j in range(len(want)) if want[j] != ct[j])
            pytest.fail("K=%d %s: first differing ct byte %d: %02x, expected %02x" % (k, name, at, ct[at], want[at]))
        assert ss.hex() == e["ss"], name
    ct_valid, ss_valid = _model_enc(model, k, *ke.valid_input(k))
    assert kf.sha3(ct_valid) == v["valid"]["ct"] and ss_valid.hex() == v["valid"]["ss"]
    for (name, ct, sk), d in zip(ke.dec_edges(k, ct_valid), v["dec"]):
        assert _model_dec(model, k, ct, sk).hex() == d["ss"], (k, name)
        mp = C.create_string_buffer(32)  # m' = indcpa_dec: what a rejection key hides
        assert model.kem_model_indcpa_dec(k, ct, sk, mp) == 0 and mp.raw.hex() == d["m"], (k, name)
    for (cond, idx, m), s in zip(ke.sampling_edges(k), v["sampling"]):
        pk, sk = kf.keypair(k, idx)
        ct, ss = _model_enc(model, k, pk, m)
        assert kf.sha3(ct) == s["ct"] and ss.hex() == s["ss"], (k, cond)
        assert _model_dec(model, k, ct, sk) == ss, (k, cond)


@pytest.mark.parametrize("k", KS)
def test_device_functions_on_the_host_reject_every_tampered_byte(model, k):  # noqa: F811
    it = kf.load()["k"]["k%d" % k][ke.TAMPER_ITEM]
    ct3, sk3 = bytes.fromhex(it["ct_hex"]), kf.keypair(k, ke.TAMPER_ITEM)[1]
    assert _model_dec(model, k, ct3, sk3).hex() == it["ss"]
    for at, t in enumerate(ke.tamper_all(ct3)):
        assert _model_dec(model, k, t, sk3) == hashlib.shake_256(sk3[-32:] + t).digest(32), (k, at)
