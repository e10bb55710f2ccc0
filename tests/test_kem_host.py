"""Kyber KEM, the part that needs no GPU: the ABI (header, api.EXPORTS, the built library), the fixture tests/golden/kem_vectors_v1.json
(re-derived from oracle/_ref where that exists -- KOSK_REQUIRE_REF=1 makes its absence a failure, as in test_oracle_vs_ref.py -- and
its internal checks everywhere), and the device functions themselves: csrc/kosk_kem_dev.hpp is host/device code, tools/kem_host_model.cpp
builds it for the host and runs a workgroup as one thread, and the result must equal the fixture item by item."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import pytest

from tests import kem_fixture as kf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (2, 3, 4)
NAMES = ["kosk_ct_bytes", "kosk_kem_enc_batch", "kosk_kem_dec_batch", "kosk_kem_enc_verified"]


def test_abi_names_and_sizes():
    from mpcith_kyber_kosk_amd import api
    hdr = open(os.path.join(ROOT, "include", "kosk_mi355x.h")).read()
    for name in NAMES:
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib, name), name
    assert "#define KOSK_SS_BYTES 32" in hdr and api.SS_BYTES == 32
    assert [api.ct_bytes(k) for k in (1, 2, 3, 4, 5)] == [0, 768, 1088, 1568, 0]
    assert [api.ct_bytes(k) for k in KS] == [kf.CT_BYTES[k] for k in KS]
    # appended: the existing ids keep their numbers
    assert api.Kosk.PATH_IDS.index("tape_expand") == 11 and api.Kosk.PATH_IDS[12:] == ["kem_enc", "kem_dec"]
    assert api.HAS_KEM


def test_fixture_shape():
    fx = kf.load()
    assert fx["format"] == "kosk-kem-v1" and fx["items"] == kf.ITEMS == 130
    for k in KS:
        items = fx["k"]["k%d" % k]
        assert len(items) == kf.ITEMS
        assert all(("ct_hex" in it) == (i < 4) for i, it in enumerate(items))
        assert [t["byte"] for t in items[3]["tampered"]] == kf.tamper_bytes(k)
        assert items[2]["noncanonical_coefficients"] > 0 and "dec_ss" in items[2]
    assert os.path.getsize(kf.PATH) < 1 << 20


@pytest.mark.parametrize("k", KS)
def test_fixture_internal_checks(k):
    """without the reference: the regenerated keys are the pinned ones, the stored ciphertexts hash to the stored digests, and every
    stored rejection key is SHAKE256(z || ct) with z from the regenerated secret key"""
    items = kf.load()["k"]["k%d" % k]
    for i, it in enumerate(items):
        pk, sk = kf.keypair(k, i)
        assert kf.sha3(pk) == it["pk"] and kf.sha3(sk) == it["sk"], i
        assert sk[384 * k:384 * k + len(pk)] == pk and sk[-64:-32] == hashlib.sha3_256(pk).digest()
        if "ct_hex" in it:
            assert kf.sha3(bytes.fromhex(it["ct_hex"])) == it["ct"] and len(it["ct_hex"]) == 2 * kf.CT_BYTES[k]
    pk2, changed = kf.noncanonical_pk(kf.keypair(k, 2)[0], k)
    assert changed == items[2]["noncanonical_coefficients"] and pk2 != kf.keypair(k, 2)[0] and len(pk2) == 384 * k + 32
    z2 = kf.keypair(k, 2)[1][-32:]
    assert items[2]["dec_ss"] == hashlib.shake_256(z2 + bytes.fromhex(items[2]["ct_hex"])).digest(32).hex() != items[2]["ss"]
    z3, ct3 = kf.keypair(k, 3)[1][-32:], bytes.fromhex(items[3]["ct_hex"])
    for t in items[3]["tampered"]:
        assert t["dec_ss"] == hashlib.shake_256(z3 + kf.tampered(ct3, t["byte"])).digest(32).hex() != items[3]["ss"]


def test_fixture_equals_reference():
    """the whole file again from oracle/_ref/libkyber_ref_k*.so"""
    missing = [p for p in (os.path.join(ROOT, "oracle", "_ref", "libkyber_ref_k%d.so" % k) for k in KS) if not os.path.exists(p)]
    if missing:
        if os.environ.get("KOSK_REQUIRE_REF") == "1":
            pytest.fail("KOSK_REQUIRE_REF=1 but %s is missing: run `make -C oracle` where the reference tree is mounted" % missing[0])
        return  # the internal checks above are what runs here
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_kem_vectors
    finally:
        sys.path.pop(0)
    assert make_kem_vectors.build() == kf.load()


@pytest.fixture(scope="module")
def model(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("kem_model") / "kem_host_model.so")
    r = subprocess.run(["c++", "-O2", "-std=c++20", "-shared", "-fPIC", "-I", os.path.join(ROOT, "mpcith_kyber_kosk_amd", "csrc"),
                        os.path.join(ROOT, "tools", "kem_host_model.cpp"), "-o", so], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return C.CDLL(so)


def test_compress_expression_exhaustive(model):
    """the device's compress() is the integer expression itself; pinned all the same, over every x in [0, q) and the four d"""
    tab = (C.c_uint16 * (4 * kf.Q))()
    model.kem_model_compress_table(tab)
    for n, d in enumerate((4, 5, 10, 11)):
        assert [tab[n * kf.Q + x] for x in range(kf.Q)] == [((x << d) + kf.Q // 2) // kf.Q % (1 << d) for x in range(kf.Q)]


@pytest.mark.parametrize("k", KS)
def test_device_functions_on_the_host_match_the_fixture(model, k):
    items = kf.load()["k"]["k%d" % k]
    ctb = kf.CT_BYTES[k]
    for i, it in enumerate(items):
        pk, sk = kf.keypair(k, i)
        ct, ss, ss2 = C.create_string_buffer(ctb), C.create_string_buffer(32), C.create_string_buffer(32)
        assert model.kem_model_enc(k, kf.enc_pk(k, i), kf.message(k, i), ct, ss) == 0
        if "ct_hex" in it and ct.raw.hex() != it["ct_hex"]:
            want = bytes.fromhex(it["ct_hex"])
            at = next(j for j in range(ctb) if want[j] != ct.raw[j])
            pytest.fail("K=%d item %d: first differing ct byte %d: %02x, expected %02x" % (k, i, at, ct.raw[at], want[at]))
        assert kf.sha3(ct.raw) == it["ct"] and ss.raw.hex() == it["ss"], i
        assert model.kem_model_dec(k, ct.raw, sk, ss2) == 0
        assert ss2.raw.hex() == (it["dec_ss"] if i == 2 else it["ss"]), i
    ct3 = bytes.fromhex(items[3]["ct_hex"])
    for t in items[3]["tampered"]:
        out = C.create_string_buffer(32)
        assert model.kem_model_dec(k, kf.tampered(ct3, t["byte"]), kf.keypair(k, 3)[1], out) == 0
        assert out.raw.hex() == t["dec_ss"]
