"""Signed heads (format kosk-headsig-v1), the parts that need no GPU: the names are declared, bound and exported, the
path ids, the hashlib model tests/headsig_model.py against the golden file, the host functions against the model byte for byte, every
tamper as the sole defect, the forgery direction that the checksum closes, the argument checks, the example under -fsyntax-only, and
tests/headsig_host_check.cpp, a stand-alone program on the host source built with ASan + UBSan."""
import ctypes as C
import hashlib
import os
import re
import shutil
import struct
import subprocess

import pytest

from tests import headsig_cases as hc
from tests import headsig_model as m

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = ["kosk_headsig_sig_bytes", "kosk_headsig_statement", "kosk_headsig_verify", "kosk_headsig_public_from_seed"]
HANDLE = ["kosk_registry_signer_reserve", "kosk_registry_signer_level", "kosk_registry_history_sign_head", "kosk_headsig_verify_heads"]
METHODS = ["registry_signer_reserve", "registry_signer_level", "registry_history_sign_head", "headsig_verify_heads"]
PROTOTYPES = (
    "size_t kosk_headsig_sig_bytes(int height);",
    "int kosk_headsig_statement(int kyber_k, const uint8_t root[32], int size, uint8_t out[56]);",
    "int kosk_headsig_verify(const uint8_t pub[52], int kyber_k, const uint8_t root[32], int size, const uint8_t *sig);",
    "int kosk_headsig_public_from_seed(int height, const uint8_t seed[32], const uint8_t id[16], uint8_t pub[52]);",
    "int kosk_registry_signer_reserve(kosk_ctx *ctx, int height, const uint8_t seed[32], const uint8_t id[16], uint8_t pub[52]);",
    "int kosk_registry_signer_level(kosk_ctx *ctx, int *height, int *has_seed);",
    "int kosk_registry_history_sign_head(kosk_ctx *ctx, int size, uint8_t *sig, uint8_t root[32], int *size_out);",
    "int kosk_headsig_verify_heads(kosk_ctx *ctx, int n, const uint8_t pub[52], const uint8_t *roots, const int32_t *sizes, const uint8_t *sigs, uint8_t *ok);",
)
HEIGHTS = (1, 2, 5)


@pytest.fixture(scope="module")
def api():
    from mpcith_kyber_kosk_amd import api
    return api


@pytest.fixture(scope="module")
def golden():
    return hc.golden()


def _header():
    return open(os.path.join(ROOT, "include", "kosk_mi355x.h")).read()


def test_names_are_declared_bound_and_exported(api):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in HOST + HANDLE:
        assert name in api.EXPORTS and hasattr(api.lib, name), name
        assert getattr(api.lib, name).argtypes is not None, name
    for method in METHODS:
        assert callable(getattr(api.Kosk, method)), method
    for fn in ("headsig_verify", "headsig_sig_bytes", "headsig_statement", "headsig_public_from_seed"):
        assert callable(getattr(api, fn)), fn
    for line in PROTOTYPES:
        assert line + "\n" in code, line
    assert "#define KOSK_HEADSIG_PUB_BYTES 52\n" in code and api.HEADSIG_PUB_BYTES == 52
    assert "#define KOSK_HEADSIG_ITEMS_PER_BLOCK %d " % api.HEADSIG_ITEMS_PER_BLOCK in code


def test_path_ids_and_the_header_sentences(api):
    K = api.Kosk
    assert (K.PATH_HEADSIG_LEAVES, K.PATH_HEADSIG_TREE, K.PATH_HEADSIG_SIGN, K.PATH_HEADSIG_VERIFY) == (49, 50, 51, 52)
    assert K.PATH_KEM_ENC_PROVEN == 48
    m_ = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int kosk_path_count\(", _header(), flags=re.S)
    text = re.sub(r"\s*\n \* ", " ", m_.group(1))
    assert "49 launches of k_headsig_leaves" in text and "50 launches of k_headsig_tree (one per tier of a build: ceil(height / 10))" in text
    assert "51 launches of k_headsig_sign (one per kosk_registry_history_sign_head" in text
    assert "52 launches of k_headsig_verify (one per launch group of kosk_headsig_verify_heads)" in text


def test_sizes(api):
    assert [api.headsig_sig_bytes(h) for h in (0, 1, 5, 24, 25, -1)] == [0, 1168, 1296, 1904, 0, 0]
    assert all(api.headsig_sig_bytes(h) == m.sig_bytes(h) == 16 + 32 + 34 * 32 + 32 * h for h in range(1, 25))


def test_model_against_the_golden_file(golden):
    """the model alone: what it computes today is what was pinned, and its own signatures verify"""
    assert golden["seed"] == hc.SEED.hex() and golden["id"] == hc.ID.hex() and golden["kyber_k"] == hc.GOLDEN_K
    for h in HEIGHTS:
        key = hc.key(h)
        assert key.pub.hex() == golden["pub"]["h%d" % h]
        for q in sorted({0, 1, (1 << h) - 1}):
            sig = key.sign(hc.GOLDEN_K, hc.golden_root(h, q), q)
            assert sig.hex() == golden["sig"]["h%d q%d" % (h, q)]
            assert len(sig) == m.sig_bytes(h) and m.verify(key.pub, hc.GOLDEN_K, hc.golden_root(h, q), q, sig) is True
    cc = golden["cross_check"]
    assert cc["x_0[0]"] == hashlib.shake_256(hc.ID + bytes(4) + bytes(2) + b"\xff" + hc.SEED).hexdigest(32)
    assert cc["C_0"] == hashlib.shake_256(hc.ID + bytes(4) + b"\xff\xfd\xff" + hc.SEED).hexdigest(32)
    assert cc["statement root 00^32 size 0 k 3"] == (b"kosk-sighead-v1\x00" + bytes(32) + struct.pack("<II", 0, 3)).hex()
    assert cc["T[1] h1"] == golden["pub"]["h1"][40:] and cc["T[1] h5"] == golden["pub"]["h5"][40:]


def test_the_documented_cross_check_values(golden):
    """INTEGRATION.md 8.10 quotes the golden file's cross-check values"""
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for v in golden["cross_check"].values():
        assert v in text, v


@pytest.mark.parametrize("h", HEIGHTS)
def test_host_functions_equal_the_model(h, api, golden):
    key = hc.key(h)
    assert api.headsig_public_from_seed(h, hc.SEED, hc.ID) == key.pub
    assert api.headsig_public_from_seed(h, hc.OTHER_SEED, hc.ID) == hc.key(h, hc.OTHER_SEED).pub != key.pub
    for q in sorted({0, 1, (1 << h) - 1}):
        root = hc.golden_root(h, q)
        sig = bytes.fromhex(golden["sig"]["h%d q%d" % (h, q)])
        for k in (2, 3, 4):
            assert api.headsig_statement(k, root, q) == m.statement(k, root, q)
            assert api.headsig_verify(key.pub, k, root, q, sig) is m.verify(key.pub, k, root, q, sig) is (k == hc.GOLDEN_K)


def test_public_key_of_height_10(api, golden):
    """the C function, proven equal to the model above, is the oracle where Python is too slow: its pinned value still stands"""
    assert api.headsig_public_from_seed(10, hc.SEED, hc.ID).hex() == golden["pub"]["h10"]
    assert golden["pub"]["h11"][:40] == (struct.pack("<I", 11) + hc.ID).hex() and golden["pub"]["h11"][40:] != golden["pub"]["h10"][40:]


@pytest.mark.parametrize("h", HEIGHTS)
def test_every_tamper_is_rejected_as_the_sole_defect(h, api, golden):
    key = hc.key(h)
    names = []
    for q in sorted({0, 1, (1 << h) - 1}):
        root = hc.golden_root(h, q)
        sig = bytes.fromhex(golden["sig"]["h%d q%d" % (h, q)])
        assert api.headsig_verify(key.pub, hc.GOLDEN_K, root, q, sig) is True
        for name, f in m.tampers(h):
            p2, r2, s2, g2 = f(key.pub, root, q, sig)
            assert (p2, r2, s2, g2) != (key.pub, root, q, sig), name
            assert m.verify(p2, hc.GOLDEN_K, r2, s2, g2) is False, (h, q, name)
            assert api.headsig_verify(p2, hc.GOLDEN_K, r2, s2, g2) is False, (h, q, name)
            names.append(name)
    assert {"C bit", "z[0] bit", "z[31] bit", "z[32] bit", "z[33] bit", "path level 0 bit", "path level h-1 bit", "root bit", "I bit", "T[1] bit",
            "q != size", "header h differs", "q = 2^h", "reserved word 0", "reserved word 1"} == set(names)


def test_an_advanced_chain_is_rejected(api, golden):
    """the forgery direction: a forger can always take z[i] further along its chain; the checksum chains would have to go backwards"""
    h, q = 5, 31
    key, root = hc.key(h), hc.golden_root(5, 31)
    sig = bytes.fromhex(golden["sig"]["h5 q31"])
    a = m.coefficients_of(key.pub, hc.GOLDEN_K, root, q, sig)
    tried = 0
    for i in range(32):
        forged = m.advance_forgery(key.pub, hc.GOLDEN_K, root, q, sig, i)
        if forged is None:
            continue
        tried += 1
        assert forged != sig and forged[48 + 32 * 32:] == sig[48 + 32 * 32:]
        assert m.verify(key.pub, hc.GOLDEN_K, root, q, forged) is False
        assert api.headsig_verify(key.pub, hc.GOLDEN_K, root, q, forged) is False
    assert tried >= 30 and len(a) == 34


def test_argument_checks(api):
    lib = api.lib
    key = hc.key(1)
    root = hc.golden_root(1, 0)
    sig = key.sign(3, root, 0)
    out = C.create_string_buffer(64)
    assert lib.kosk_headsig_verify(key.pub, 3, root, 0, sig) == 1
    assert lib.kosk_headsig_verify(None, 3, root, 0, sig) == -1 and lib.kosk_headsig_verify(key.pub, 3, None, 0, sig) == -1
    assert lib.kosk_headsig_verify(key.pub, 3, root, 0, None) == -1 and lib.kosk_headsig_verify(key.pub, 3, root, -1, sig) == -1
    for k in (1, 5, 0, -3):
        assert lib.kosk_headsig_verify(key.pub, k, root, 0, sig) == -1
        assert lib.kosk_headsig_statement(k, root, 0, out) == -1
    for h in (0, 25, 0xFFFFFFFF):
        assert lib.kosk_headsig_verify(struct.pack("<I", h) + key.pub[4:], 3, root, 0, sig) == -1
    assert lib.kosk_headsig_statement(3, None, 0, out) == -1 and lib.kosk_headsig_statement(3, root, -1, out) == -1
    assert lib.kosk_headsig_statement(3, root, 0, None) == -1
    for h in (0, 25, -1):
        assert lib.kosk_headsig_public_from_seed(h, hc.SEED, hc.ID, out) == -1
    assert lib.kosk_headsig_public_from_seed(1, None, hc.ID, out) == -1 and lib.kosk_headsig_public_from_seed(1, hc.SEED, None, out) == -1
    assert lib.kosk_headsig_public_from_seed(1, hc.SEED, hc.ID, None) == -1
    assert out.raw == bytes(64)
    buf = C.create_string_buffer(4096)
    sizes = (C.c_int32 * 1)(0)
    assert lib.kosk_registry_signer_reserve(None, 1, hc.SEED, hc.ID, buf) == -1 and lib.kosk_registry_signer_level(None, None, None) == -1
    assert lib.kosk_registry_history_sign_head(None, 0, buf, buf, None) == -1
    assert lib.kosk_headsig_verify_heads(None, 1, key.pub, buf, sizes, buf, buf) == -1
    assert buf.raw == bytes(4096)


def test_the_example_parses():
    """examples/registry_signed.cpp against the header, host side only"""
    cxx = shutil.which("hipcc") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    cmd = [cxx, "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "registry_signed.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout


def test_headsig_host_check(tmp_path):
    """the host source under ASan + UBSan in a stand-alone program: key generation at heights 1 and 2, a signer written there, every size
    signed and verified from unaligned buffers, every tamper, the refusals"""
    exe = str(tmp_path / "headsig_host_check")
    r = subprocess.run(["c++", "-std=c++20", "-O2", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "mpcith_kyber_kosk_amd", "csrc"), os.path.join(ROOT, "tests", "headsig_host_check.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    m_ = re.search(r"headsig checks (\d+) failures 0\n", r.stdout)
    assert r.returncode == 0 and m_ and int(m_.group(1)) >= 250 and "FAILED" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
