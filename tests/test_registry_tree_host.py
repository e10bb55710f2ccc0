"""The registry tree, format kosk-regtree-v1, the parts that need no GPU: the eight names are declared, bound and
exported, the three path ids and the header's sentences for them, kosk_registry_tree_depth / _bytes, kosk_regtree_leaf / _node /
_root_from_path against the hashlib model of tests/registry_tree_model.py, every refusal of the host functions, the example under
-fsyntax-only, and tests/regtree_host_check.cpp, a stand-alone program on the host source built with ASan + UBSan."""
import ctypes as C
import hashlib
import os
import random
import re
import shutil
import subprocess

import pytest

from tests import registry_tree_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kosk_registry_tree_depth", "kosk_registry_tree_bytes", "kosk_regtree_leaf", "kosk_regtree_node", "kosk_regtree_root_from_path",
         "kosk_registry_root", "kosk_registry_prove_slots", "kosk_registry_prove_peers"]
METHODS = ["registry_root", "registry_prove_slots", "registry_prove_peers"]
FUNCTIONS = ["registry_tree_depth", "registry_tree_bytes", "regtree_leaf", "regtree_node", "regtree_root_from_path"]
# capacity -> D
DEPTHS = {1: 0, 2: 1, 3: 2, 4: 2, 5: 3, 1024: 10, 1025: 11, 2 ** 20: 20, 2 ** 20 + 1: 21}


@pytest.fixture(scope="module")
def api():
    from mpcith_kyber_kosk_amd import api
    return api


def _header():
    return open(os.path.join(ROOT, "include", "kosk_mi355x.h")).read()


def test_the_model_pins_the_empty_leaves():
    for k in (2, 3, 4):
        assert tm.empty(k) == tm.EMPTY[k] == hashlib.sha3_256(b"kosk-regtree-v1\x01" + bytes([k, 0, 0, 0])).digest()
    assert (tm.EMPTY[2].hex()[:8], tm.EMPTY[3].hex()[:8], tm.EMPTY[4].hex()[:8]) == ("2aca555f", "dd6d2c3c", "a93686a2")
    # the sparse form of the model is the dense one
    content = {0: bytes(32), 3: b"\x01" * 32, 4: b"\x02" * 32}
    lv = tm.levels(2, 5, content)
    sp, blank = tm.sparse_root(2, 5, content)
    assert sp[-1][0] == tm.root(lv) and all(tm.sparse_path(sp, blank, s) == tm.path(lv, s) for s in range(8))
    assert len(lv) == 4 and [len(x) for x in lv] == [8, 4, 2, 1]


def test_names_are_declared_bound_and_exported(api):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b(?:int|size_t) %s\s*\(" % name, code), name
        assert name in api.EXPORTS and hasattr(api.lib, name), name
        assert getattr(api.lib, name).argtypes is not None, name
    for method in METHODS:
        assert callable(getattr(api.Kosk, method)), method
    for fn in FUNCTIONS:
        assert callable(getattr(api, fn)), fn
    assert re.search(r"int kosk_registry_root\(kosk_ctx \*ctx, uint8_t root\[32\], int \*used, int \*capacity\);", code)
    assert re.search(r"int kosk_registry_prove_slots\(kosk_ctx \*ctx, int n, const int32_t \*slots, uint8_t \*state, uint8_t \*h, "
                     r"uint8_t \*paths, uint8_t \*root\);", code)
    assert re.search(r"int kosk_registry_prove_peers\(kosk_ctx \*ctx, int n, const uint8_t \*h, int32_t \*slots, uint8_t \*paths, "
                     r"uint8_t \*done, uint8_t \*root\);", code)
    assert re.search(r"int kosk_regtree_root_from_path\(int kyber_k, int depth, int32_t slot, const uint8_t \*h, const uint8_t \*path, "
                     r"uint8_t root\[32\]\);", code)
    assert re.search(r"enum \{ KOSK_REGTREE_TIER_LEVELS = 10 \};", code) and api.REGTREE_TIER_LEVELS == 10


def test_path_ids_and_the_header_sentences(api):
    assert (api.Kosk.PATH_REGISTRY_TREE, api.Kosk.PATH_REGISTRY_SUBTREES, api.Kosk.PATH_REGISTRY_PATH) == (32, 33, 34)
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int kosk_path_count\(", _header(), flags=re.S)
    assert m
    text = re.sub(r"\s*\n \* ", " ", m.group(1))
    assert "32 launches of k_registry_tree (one per tier of a rebuild)" in text
    assert "33 leaf subtrees hashed by those launches" in text
    assert "34 launches of k_registry_path (one per launch group of kosk_registry_prove_slots / kosk_registry_prove_peers)" in text
    # the earlier sentences are still there, word for word
    assert re.search(r"\b27 launches of k_registry_admit\b", text) and re.search(r"\b28 kem_enc_slots\b", text)
    assert re.search(r"\b29 launches of k_registry_index\b", text) and re.search(r"\b30 launches of k_registry_find\b", text)
    assert re.search(r"\b31 kem_enc_peers\b", text)


def test_depth_and_bytes(api):
    for capacity, d in DEPTHS.items():
        assert api.registry_tree_depth(capacity) == d == tm.depth(capacity), capacity
        assert api.registry_tree_bytes(capacity) == (2 * 2 ** d - 1) * 32 == tm.tree_bytes(capacity), capacity
    for capacity in (0, -1):
        assert api.registry_tree_depth(capacity) == -1 == tm.depth(capacity)
        assert api.registry_tree_bytes(capacity) == 0 == tm.tree_bytes(capacity)


def test_leaf_and_node_against_the_model(api):
    rng = random.Random(20250)
    for i in range(300):
        k = 2 + i % 3
        h, l, r = (rng.randbytes(32) for _ in range(3))
        assert api.regtree_leaf(k, h) == tm.leaf(k, h), i
        assert api.regtree_node(l, r) == tm.node(l, r), i
    for k in (2, 3, 4):
        assert api.regtree_leaf(k) == tm.EMPTY[k]
        assert api.regtree_leaf(k, bytes(32)) == tm.leaf(k, bytes(32)) != tm.EMPTY[k]


@pytest.mark.parametrize("d", (0, 1, 11, 31))
def test_root_from_path_against_the_model(d, api):
    rng = random.Random(31 + d)
    edge = [0, (1 << d) - 1]
    for i in range(100):
        k = 2 + i % 3
        slot = edge[i] if i < 2 else rng.randrange(1 << d)
        h = None if i % 4 == 3 else rng.randbytes(32)
        p = rng.randbytes(32 * d)
        want = tm.root_from_path(k, d, slot, h, p)
        assert api.regtree_root_from_path(k, d, slot, h, p) == want, (d, i)
        if d:
            flipped = bytearray(p)
            flipped[rng.randrange(len(p))] ^= 1 << rng.randrange(8)
            assert api.regtree_root_from_path(k, d, slot, h, bytes(flipped)) != want
        else:
            assert want == (tm.empty(k) if h is None else tm.leaf(k, h))


def test_whole_trees_against_the_model(api):
    """leaf, node and root_from_path of the library rebuild the model's tree at capacities 1, 3 and 5 and walk every path"""
    for k, capacity, occupied in ((2, 1, [0]), (3, 3, [0, 2]), (4, 5, [1, 4]), (2, 5, [])):
        content = {s: hashlib.sha3_256(b"tree-host:%d:%d" % (capacity, s)).digest() for s in occupied}
        lv = tm.levels(k, capacity, content)
        d = tm.depth(capacity)
        got = [[api.regtree_leaf(k, content.get(s)) for s in range(1 << d)]]
        for l in range(d):
            got.append([api.regtree_node(got[l][2 * i], got[l][2 * i + 1]) for i in range(len(got[l]) // 2)])
        assert got == lv
        for s in range(1 << d):
            assert api.regtree_root_from_path(k, d, s, content.get(s), tm.path(lv, s)) == tm.root(lv)


def test_refusals_of_the_host_functions(api):
    lib = api.lib
    a, out, path = C.create_string_buffer(32), C.create_string_buffer(32), C.create_string_buffer(64)
    assert lib.kosk_regtree_leaf(1, a, out) == -1 and lib.kosk_regtree_leaf(5, None, out) == -1 and lib.kosk_regtree_leaf(2, a, None) == -1
    assert lib.kosk_regtree_node(None, a, out) == -1 and lib.kosk_regtree_node(a, None, out) == -1 and lib.kosk_regtree_node(a, a, None) == -1
    rfp = lib.kosk_regtree_root_from_path
    assert rfp(1, 1, 0, a, path, out) == -1 and rfp(5, 1, 0, a, path, out) == -1            # bad k
    assert rfp(2, -1, 0, a, path, out) == -1 and rfp(2, 32, 0, a, path, out) == -1          # depth outside 0..31
    assert rfp(2, 1, -1, a, path, out) == -1 and rfp(2, 1, 2, a, path, out) == -1           # slot outside [0, 2^depth)
    assert rfp(2, 0, 1, a, None, out) == -1 and rfp(2, 31, -2 ** 31, a, path, out) == -1
    assert rfp(2, 1, 0, a, path, None) == -1 and rfp(2, 1, 0, a, None, out) == -1           # NULL out, NULL path with depth > 0
    assert rfp(2, 0, 0, a, None, out) == 0 and out.raw == tm.leaf(2, bytes(32))             # depth 0 needs no path
    assert rfp(2, 2, 3, None, path, out) == 0 and out.raw == tm.root_from_path(2, 2, 3, None, bytes(64))
    # the handle calls without a handle
    slots = (C.c_int32 * 2)(0, 1)
    assert lib.kosk_registry_root(None, out, None, None) == -1
    assert lib.kosk_registry_prove_slots(None, 1, slots, a, a, path, out) == -1
    assert lib.kosk_registry_prove_peers(None, 1, a, slots, path, a, out) == -1
    with pytest.raises(api.KoskError):
        api.regtree_leaf(5)
    with pytest.raises(api.KoskError):
        api.regtree_root_from_path(2, 2, 4, None, bytes(64))
    with pytest.raises(api.KoskError):
        api.regtree_root_from_path(2, 2, 0, None, bytes(63))


def test_the_example_parses():
    """examples/registry_audit.cpp against the header, host side only"""
    cxx = shutil.which("hipcc") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    cmd = [cxx, "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "registry_audit.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout


def test_regtree_host_check(tmp_path):
    """the host source under ASan + UBSan in a stand-alone program: paths at depths 0 and 31, the refusals"""
    exe = str(tmp_path / "regtree_host_check")
    r = subprocess.run(["c++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "mpcith_kyber_kosk_amd", "csrc"), os.path.join(ROOT, "tests", "regtree_host_check.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    m = re.search(r"regtree checks (\d+) failures 0\n", r.stdout)
    assert r.returncode == 0 and m and int(m.group(1)) >= 200 and "FAILED" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
