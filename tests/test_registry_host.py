"""The verified-key registry, the parts that need no GPU: the eight names are declared, bound and exported, the two
path ids and the header's sentences for them, kosk_registry_slot_bytes, the NULL-argument returns, the example under -fsyntax-only and
the injectivity of the slot maps of tests/registry_cases.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from tests import registry_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kosk_registry_slot_bytes", "kosk_registry_reserve", "kosk_registry_level", "kosk_registry_admit_verified", "kosk_registry_admit",
         "kosk_registry_evict", "kosk_registry_read", "kosk_kem_enc_slots"]
METHODS = ["registry_reserve", "registry_level", "registry_admit_verified", "registry_admit", "registry_evict", "registry_read", "kem_enc_slots"]


@pytest.fixture(scope="module")
def api():
    from mpcith_kyber_kosk_amd import api
    return api


def _header():
    return open(os.path.join(ROOT, "include", "kosk_mi355x.h")).read()


def test_names_are_declared_bound_and_exported(api):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b(?:int|size_t) %s\s*\(" % name, code), name
        assert name in api.EXPORTS and hasattr(api.lib, name), name
        assert getattr(api.lib, name).argtypes is not None, name
    for method in METHODS:
        assert callable(getattr(api.Kosk, method)), method
    assert re.search(r"int kosk_kem_enc_slots\(kosk_ctx \*ctx, int n, const int32_t \*slots, const uint8_t \*coins, uint8_t \*ct, uint8_t \*ss, "
                     r"uint8_t \*done\);", code)
    assert re.search(r"int kosk_registry_admit\(kosk_ctx \*ctx, int n, const uint8_t \*pk, const uint8_t \*accept, const int32_t \*slots\);", code)


def test_path_ids_and_the_header_sentences(api):
    assert (api.Kosk.PATH_REGISTRY_ADMIT, api.Kosk.PATH_KEM_ENC_SLOTS) == (27, 28)
    assert api.Kosk.PATH_IDS[-1] == "kem_dec" and len(api.Kosk.PATH_IDS) == 14  # that list stays as it is
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int kosk_path_count\(", _header(), flags=re.S)
    assert m
    text = m.group(1)
    assert re.search(r"\b27 launches of k_registry_admit\b", text) and re.search(r"\b28 kem_enc_slots\b", text)
    # the earlier sentences are still there, word for word
    assert re.search(r"\b19 launches of k_kem_key_setup\b", text) and re.search(r"\b20 kem_enc_key / 21 kem_dec_key\b", text)
    assert re.search(r"\b25 launches of k_bank_put\b", text) and re.search(r"\b26 launches of k_bank_take\b", text)


def test_slot_bytes(api):
    """pk bytes (384 K + 32) + H(pk) (32) + A^T (K^2 polynomials of 256 int16) + the flag; 0 for a k that is no parameter set"""
    want = {1: 0, 2: 800 + 32 + 4 * 512 + 1, 3: 1184 + 32 + 9 * 512 + 1, 4: 1568 + 32 + 16 * 512 + 1, 5: 0}
    for k in range(1, 6):
        assert api.registry_slot_bytes(k) == want[k], k
    assert [round(want[k] / 1000, 1) for k in rc.KS] == [2.9, 5.8, 9.8]


def test_null_arguments_return_minus_one(api):
    lib = api.lib
    buf = C.create_string_buffer(64)
    slots = (C.c_int32 * 2)(0, 1)
    assert lib.kosk_registry_reserve(None, 4) == -1
    assert lib.kosk_registry_level(None, None, None) == -1
    assert lib.kosk_registry_admit_verified(None, 1, slots, buf) == -1
    assert lib.kosk_registry_admit(None, 1, buf, None, slots) == -1
    assert lib.kosk_registry_evict(None, 1, slots) == -1
    assert lib.kosk_registry_read(None, 1, slots, buf, None, None) == -1
    assert lib.kosk_kem_enc_slots(None, 1, slots, buf, buf, buf, buf) == -1


def test_the_example_parses():
    """examples/registry_enrol.cpp against the header, host side only"""
    cxx = shutil.which("hipcc") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    cmd = [cxx, "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "registry_enrol.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout


def test_the_slot_maps_are_injective():
    small = [rc.slot(i) for i in range(130)]
    assert len(set(small)) == 130 and min(small) >= 0 and max(small) < rc.CAPACITY
    assert rc.slot(97) == 0 and rc.slot(24) == rc.CAPACITY - 1  # both ends of the registry are used
    edge = [rc.edge_slot(b) for b in range(rc.WAVE_MAX + 1)]
    assert len(set(edge)) == rc.WAVE_MAX + 1 and min(edge) >= 0 and max(edge) < rc.EDGE_CAPACITY
    big = [rc.big_slot(b) for b in range(rc.CHUNK + 1)]
    assert len(set(big)) == rc.CHUNK + 1 and min(big) >= 0 and max(big) < rc.BIG_CAPACITY
    assert rc.big_slot(rc.CHUNK) != rc.big_slot(0)  # an offset into `slots` that restarts at a launch group lands on another key's slot
