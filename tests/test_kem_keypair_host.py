"""KEM key pairs and key checks, the part that needs no GPU: the ABI (header, api.EXPORTS, the built library, the compat header), the
fixture tests/golden/kem_keypair_v1.json (re-derived from oracle/_ref where that exists -- KOSK_REQUIRE_REF=1 makes its absence a
failure), the model the GPU tests compare with (tests/kem_keypair_cases.py: api.host_keygen with z in the last 32 bytes) against every
digest of the fixture, and the device functions themselves: csrc/kosk_kem_dev.hpp is host/device code, tools/kem_keypair_host_model.cpp
runs a workgroup as one thread.  Every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import pytest

from tests import kem_keypair_cases as kk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = kk.KS
NAMES = ["kosk_kem_keypair_batch", "kosk_kem_check_pk", "kosk_kem_check_sk"]


def test_abi_names():
    from mpcith_kyber_kosk_amd import api
    hdr = open(os.path.join(ROOT, "include", "kosk_mi355x.h")).read()
    for name in NAMES:
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib, name), name
    for name in ("kem_keypair", "kem_check_pk", "kem_check_sk"):
        assert callable(getattr(api.Kosk, name))
    assert (api.Kosk.PATH_DENSE_FILL, api.Kosk.PATH_KEM_KEYPAIR, api.Kosk.PATH_KEM_CHECK) == (14, 15, 16)
    assert api.Kosk.PATH_IDS[-1] == "kem_dec"  # the list that path_counts() walks stays as it is
    assert (api.KEYCHK_HASH, api.KEYCHK_PK_RANGE, api.KEYCHK_S_RANGE) == (kk.HASH, kk.PK_RANGE, kk.S_RANGE) == (1, 2, 4)
    for name, v in (("KOSK_KEYCHK_HASH", 1), ("KOSK_KEYCHK_PK_RANGE", 2), ("KOSK_KEYCHK_S_RANGE", 4)):
        assert "#define %s" % name in hdr and ("#define %-20s %d" % (name, v)) in hdr, name
    compat = open(os.path.join(ROOT, "include", "kosk_compat.hpp")).read()
    assert "crypto_kem_keypair_derand(" in compat and "crypto_kem_keypair(" in compat


@pytest.mark.parametrize("k", KS)
def test_model_reproduces_the_fixture(k):
    """the reference's keypair_derand, as recorded, is api.host_keygen with z in the last 32 bytes -- for all 130 items"""
    fx = kk.load()["k"]["k%d" % k]
    assert kk.load()["items"] == kk.ITEMS == len(fx["items"])
    for i, rec in enumerate(fx["items"]):
        pk, sk = kk.keypair(k, i)
        assert len(pk) == 384 * k + 32 and len(sk) == 768 * k + 96
        assert kk.sha3(pk) == rec["pk"] and kk.sha3(sk) == rec["sk"], (k, i)
        assert sk[-32:] == kk.coins(k, i)[32:]
    four = [i for i in range(kk.ITEMS) if kk.needs_fourth_block(k, kk.coins(k, i))]
    assert four == fx["four_block"] and four


def test_fixture_equals_reference():
    """the whole file again from oracle/_ref/libkyber_ref_k*.so"""
    missing = [p for p in (os.path.join(ROOT, "oracle", "_ref", "libkyber_ref_k%d.so" % k) for k in KS) if not os.path.exists(p)]
    if missing:
        if os.environ.get("KOSK_REQUIRE_REF") == "1":
            pytest.fail("KOSK_REQUIRE_REF=1 but %s is missing: run `make -C oracle` where the reference tree is mounted" % missing[0])
        return  # the digests above are what runs here
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_kem_keypair_vectors
    finally:
        sys.path.pop(0)
    assert make_kem_keypair_vectors.build() == kk.load()


@pytest.mark.parametrize("k", KS)
def test_compat_header_compiles(k):
    """crypto_kem_keypair_derand / crypto_kem_keypair next to the rest of kyber/kem.h, used the way a caller of the reference uses them"""
    src = ('#include "kosk_compat.hpp"\n'
           "int f(uint8_t *pk, uint8_t *sk, const uint8_t *coins, uint8_t *ct, uint8_t *ss) {\n"
           "  static_assert(KYBER_PUBLICKEYBYTES == %d && KYBER_SECRETKEYBYTES == %d, \"sizes\");\n"
           "  int r = crypto_kem_keypair_derand(pk, sk, coins) | crypto_kem_keypair(pk, sk);\n"
           "  return r | crypto_kem_enc(ct, ss, pk) | crypto_kem_dec(ss, ct, sk); }\n" % (384 * k + 32, 768 * k + 96))
    r = subprocess.run(["c++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-DKYBER_K=%d" % k, "-I", os.path.join(ROOT, "include"), "-x", "c++", "-"],
                       input=src, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]


@pytest.mark.parametrize("k", KS)
def test_flag_model(k):
    """0 on every fixture key; each flag alone and together on hand-made records"""
    pvb = 384 * k
    for i in range(kk.ITEMS):
        pk, sk = kk.keypair(k, i)
        assert kk.flags_pk(k, pk) == 0 and kk.flags_sk(k, sk) == 0, (k, i)
    pk, sk = kk.keypair(k, 0)
    assert kk.fields(kk.set_field(pk, 0, 5, kk.Q))[5] == kk.Q and kk.fields(kk.set_field(pk, 0, 4, 0xFFF))[3:6] == kk.fields(pk)[3:4] + [0xFFF] + kk.fields(pk)[5:6]
    assert kk.flags_pk(k, kk.set_field(pk, 0, 256 * k - 1, kk.Q)) == kk.PK_RANGE and kk.flags_pk(k, kk.set_field(pk, 0, 0, kk.Q - 1)) == 0
    assert kk.flags_sk(k, kk.set_field(sk, 0, 7, kk.Q)) == kk.S_RANGE
    assert kk.flags_sk(k, kk.set_field(sk, pvb, 7, kk.Q - 1)) == kk.HASH
    assert kk.flags_sk(k, kk.set_field(sk, pvb, 7, kk.Q)) == kk.HASH | kk.PK_RANGE
    assert kk.flags_sk(k, kk.flip(sk, len(sk) - 33)) == kk.HASH and kk.flags_sk(k, kk.flip(sk, len(sk) - 1)) == 0


@pytest.fixture(scope="module")
def device_model(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("kem_keypair_model") / "kem_keypair_host_model.so")
    r = subprocess.run(["c++", "-O2", "-std=c++20", "-shared", "-fPIC", "-I", os.path.join(ROOT, "mpcith_kyber_kosk_amd", "csrc"),
                        os.path.join(ROOT, "tools", "kem_keypair_host_model.cpp"), "-o", so], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return C.CDLL(so)


@pytest.mark.parametrize("k", KS)
def test_device_functions_on_the_host(device_model, k):
    """seed_hash_g, matrix_entry (not transposed), noise_poly, keypair_block and range12x8 as the kernels call them: every fixture
    item byte for byte, the block limit on the four-block items, and the check flags on tampered records"""
    fx = kk.load()["k"]["k%d" % k]
    pvb = 384 * k
    for i in range(kk.ITEMS):
        want_pk, want_sk = kk.keypair(k, i)
        pk, sk = C.create_string_buffer(len(want_pk)), C.create_string_buffer(len(want_sk))
        assert device_model.kem_model_keypair(k, 32, kk.coins(k, i), pk, sk) == 0
        for what, got, want in (("pk", pk.raw, want_pk), ("sk", sk.raw, want_sk)):
            if got != want:
                at = next(j for j in range(len(want)) if got[j] != want[j])
                pytest.fail("K=%d item %d: first differing %s byte %d: %02x, expected %02x" % (k, i, what, at, got[at], want[at]))
        assert device_model.kem_model_keypair(k, 3, kk.coins(k, i), pk, sk) == (-2 if i in fx["four_block"] else 0), (k, i)
        assert device_model.kem_model_check(k, 0, want_pk) == 0 and device_model.kem_model_check(k, 1, want_sk) == 0
    pk, sk = kk.keypair(k, 1)
    recs = [kk.set_field(sk, at, f, v) for at in (0, pvb) for f in (0, 1, 255, 256, 256 * k - 1) for v in (kk.Q - 1, kk.Q, 0xFFF)]
    recs += [kk.flip(sk, b) for b in (pvb + 3, 2 * pvb, 2 * pvb + 31, 2 * pvb + 32, 2 * pvb + 63, 2 * pvb + 64, len(sk) - 1)]
    for rec in recs:
        assert device_model.kem_model_check(k, 1, rec) == kk.flags_sk(k, rec)
        assert device_model.kem_model_check(k, 0, rec[pvb:2 * pvb + 32]) == kk.flags_pk(k, rec[pvb:2 * pvb + 32])
