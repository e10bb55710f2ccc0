"""The registry by fingerprint, the parts that need no GPU: the seven names are declared, bound and exported, the
three path ids and the header's sentences for them, kosk_registry_index_entries and kosk_registry_index_home against the model of
tests/registry_index_model.py, the NULL-argument returns, the example under -fsyntax-only, and the model's own checks: grind() delivers the
homes it promises, and the enrol rule on hand-written cases."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess

import pytest

from tests import registry_index_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kosk_registry_index_entries", "kosk_registry_index_home", "kosk_registry_find", "kosk_registry_enrol_verified",
         "kosk_registry_enrol", "kosk_kem_enc_peers"]
METHODS = ["registry_find", "registry_enrol", "registry_enrol_verified", "kem_enc_peers"]
# capacity -> T, the smallest power of two >= 2 x capacity.  2 x 16 400 = 32 800 lies above 32 768, so that registry gets 65 536 entries:
# with 32 768 its load could pass 1/2, which the definition rules out
CAPACITIES = {1: 2, 2: 4, 3: 8, 4: 8, 5: 16, 300: 1024, 16400: 65536}


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
    assert callable(api.registry_index_entries) and callable(api.registry_index_home)
    # the seventh name is the enum
    assert re.search(r"enum \{ KOSK_ENROL_REJECTED = 0, KOSK_ENROL_ADMITTED = 1, KOSK_ENROL_DUPLICATE = 2 \};", code)
    assert (api.ENROL_REJECTED, api.ENROL_ADMITTED, api.ENROL_DUPLICATE) == (0, 1, 2) == (rm.REJECTED, rm.ADMITTED, rm.DUPLICATE)
    assert re.search(r"int kosk_kem_enc_peers\(kosk_ctx \*ctx, int n, const uint8_t \*h, const uint8_t \*coins, uint8_t \*ct, uint8_t \*ss, "
                     r"uint8_t \*done\);", code)
    assert re.search(r"int kosk_registry_enrol\(kosk_ctx \*ctx, int n, const uint8_t \*pk, const uint8_t \*accept, int32_t \*slots, "
                     r"uint8_t \*status\);", code)
    assert re.search(r"int kosk_registry_enrol_verified\(kosk_ctx \*ctx, int n, int32_t \*slots, uint8_t \*status\);", code)
    assert re.search(r"int kosk_registry_find\(kosk_ctx \*ctx, int n, const uint8_t \*h, int32_t \*slots\);", code)


def test_path_ids_and_the_header_sentences(api):
    assert (api.Kosk.PATH_REGISTRY_INDEX, api.Kosk.PATH_REGISTRY_FIND, api.Kosk.PATH_KEM_ENC_PEERS) == (29, 30, 31)
    assert (api.Kosk.PATH_REGISTRY_ADMIT, api.Kosk.PATH_KEM_ENC_SLOTS) == (27, 28)
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int kosk_path_count\(", _header(), flags=re.S)
    assert m
    text = m.group(1)
    assert re.search(r"\b29 launches of k_registry_index\b", text) and re.search(r"\b30 launches of k_registry_find\b", text)
    assert re.search(r"\b31 kem_enc_peers\b", text)
    # the earlier sentences are still there, word for word
    assert re.search(r"\b27 launches of k_registry_admit\b", text) and re.search(r"\b28 kem_enc_slots\b", text)


def test_index_entries(api):
    for capacity, want in CAPACITIES.items():
        assert api.registry_index_entries(capacity) == want == rm.entries(capacity), capacity
    for capacity in (0, -1, -(2 ** 31)):
        assert api.registry_index_entries(capacity) == 0 == rm.entries(capacity)


def test_index_home_against_the_model(api):
    hs = [hashlib.shake_256(b"registry-home:%d" % i).digest(32) for i in range(1000)]
    for capacity, t in CAPACITIES.items():
        got = [api.registry_index_home(capacity, h) for h in hs]
        assert got == [rm.home(capacity, h) for h in hs], capacity
        assert min(got) >= 0 and max(got) < t
    assert rm.home(1, b"\x01" + bytes(31)) == 1 and rm.home(300, b"\xff\xff\xff\xff" + bytes(28)) == 1023
    assert rm.home(300, bytes([0x34, 0x12]) + bytes(30)) == 0x234  # little endian
    assert api.registry_index_home(0, hs[0]) == -1 and api.registry_index_home(-5, hs[0]) == -1


def test_null_arguments_return_minus_one(api):
    lib = api.lib
    buf = C.create_string_buffer(64)
    slots = (C.c_int32 * 2)(0, 1)
    assert lib.kosk_registry_index_home(4, None) == -1
    assert lib.kosk_registry_find(None, 1, buf, slots) == -1
    assert lib.kosk_registry_enrol_verified(None, 1, slots, buf) == -1
    assert lib.kosk_registry_enrol(None, 1, buf, None, slots, buf) == -1
    assert lib.kosk_kem_enc_peers(None, 1, buf, buf, buf, buf, buf) == -1


def test_the_example_parses():
    """examples/registry_peers.cpp against the header, host side only"""
    cxx = shutil.which("hipcc") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    cmd = [cxx, "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "registry_peers.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout


def test_grind_delivers_the_homes_it_promises():
    """the GPU cases rely on these collisions: at every capacity they use, on every home they use, distinct keys with that home"""
    for capacity, size in ((1, 800), (2, 800), (3, 800), (8, 800)):
        t = rm.entries(capacity)
        for target in (0, t - 1, t // 2):
            keys = rm.grind(capacity, target, capacity + 2, size)
            assert len(set(keys)) == capacity + 2 and all(len(pk) == size for pk in keys)
            assert [rm.home(capacity, rm.fp(pk)) for pk in keys] == [target] * (capacity + 2)
            other = rm.grind(capacity, target, 2, size, tag=b"absent")
            assert not set(other) & set(keys) and [rm.home(capacity, rm.fp(pk)) for pk in other] == [target] * 2


def test_the_enrol_rule():
    a, b, c, d, e = (bytes([i]) * 8 for i in range(5))
    m = rm.Model(4)
    m.admit([a], [1])
    # a rejected first occurrence does not count: the second occurrence of b is admitted, the third is its duplicate
    assert m.enrol([b, b, a, b, c], accept=[0, 1, 1, 1, 1]) == ([-1, 0, 1, 0, 2], [rm.REJECTED, rm.ADMITTED, rm.DUPLICATE, rm.DUPLICATE, rm.ADMITTED])
    assert m.slots == [b, a, c, None] and m.find(rm.fp(b)) == 0 and m.find(rm.fp(d)) == -1
    # a full registry: two new keys, one empty slot; nothing changes
    before = list(m.slots)
    assert m.enrol([d, e]) is None and m.slots == before
    assert m.enrol([d, d, a]) == ([3, 3, 1], [rm.ADMITTED, rm.DUPLICATE, rm.DUPLICATE])
    # duplicates through admit: find gives the lowest slot
    m.evict([0, 2])
    m.admit([a], [2])
    assert m.find(rm.fp(a)) == 1 and m.table()[rm.fp(a)] == [1, 2]
    m.evict([1])
    assert m.find(rm.fp(a)) == 2
