"""The registry history, format kosk-reghist-v1, the parts that need no GPU: the fifteen names are declared, bound and
exported, the four path ids and the header's sentences for them, the size functions, kosk_reghist_leaf / _node / _empty_root /
_root_from_path / _check_consistency against the recursive hashlib model of tests/registry_history_model.py for every (i, n) and (m, n)
with n <= 70, every rule of both verifiers as the sole reason to reject, every refusal of the host functions, the example under
-fsyntax-only, and tests/reghist_host_check.cpp, a stand-alone program on the host source built with ASan + UBSan."""
import ctypes as C
import hashlib
import os
import random
import re
import shutil
import struct
import subprocess

import pytest

from tests import registry_history_model as hm
from tests import registry_sorted_model as sm
from tests import registry_tree_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = ["kosk_reghist_depth", "kosk_reghist_path_bytes", "kosk_reghist_consistency_bytes", "kosk_reghist_leaf", "kosk_reghist_node",
        "kosk_reghist_empty_root", "kosk_reghist_root_from_path", "kosk_reghist_check_consistency"]
HANDLE = ["kosk_registry_history_reserve", "kosk_registry_history_level", "kosk_registry_history_head", "kosk_registry_history_checkpoint",
          "kosk_registry_history_read", "kosk_registry_history_prove_events", "kosk_registry_history_prove_consistency"]
METHODS = ["registry_history_reserve", "registry_history_level", "registry_history_head", "registry_history_checkpoint",
           "registry_history_read", "registry_history_prove_events", "registry_history_prove_consistency"]
FUNCTIONS = ["reghist_depth", "reghist_path_bytes", "reghist_consistency_bytes", "reghist_leaf", "reghist_node", "reghist_empty_root",
             "reghist_root_from_path", "reghist_check_consistency", "reghist_event"]
ZERO, ONES = bytes(32), b"\xff" * 32
NMAX = 70


@pytest.fixture(scope="module")
def api():
    from mpcith_kyber_kosk_amd import api
    return api


@pytest.fixture(scope="module")
def leaves():
    return [hashlib.sha3_256(b"history-host:%d" % i).digest() for i in range(NMAX)]


def _header():
    return open(os.path.join(ROOT, "include", "kosk_mi355x.h")).read()


def test_the_model_pins_the_six_digests():
    for k in (2, 3, 4):
        assert hm.empty(k).hex() == hm.PINS["O%d" % k]
        assert hm.empty(k) == hashlib.sha3_256(b"kosk-reghist-v1\x03" + bytes([k, 0, 0, 0])).digest()
    assert hm.event_leaf(3, ZERO, hm.ADMIT, 0).hex() == hm.PINS["V"] == "a072946f099b63a9511d962e7ec11810ff0170e9188caa33afe7ef116fa8f989"
    assert hm.checkpoint_leaf(3, ZERO, ONES, 0, 1).hex() == hm.PINS["C"] == "c3ac69cab994754912dc117aab3f76ccc0047ff5af0207138ac8aa4228f221f8"
    assert hm.node(ZERO, ONES).hex() == hm.PINS["N"] == "a94fdaf8f5573f9a257629c4d09419ae82d0d3bcfe77ab04f1f947cf628ca528"
    assert hm.PINS["O2"] == "d8a55b610cc5228141b2f211b388d4bfc4c5aea61aa6496c031c1be6b52acbfb"
    assert hm.PINS["O3"] == "3bbed6e89d035147e6e7ad59edb52a42a5610bd4b48ac5f302f713848ebe91f3"
    assert hm.PINS["O4"] == "5aa09ad7d3d4c522d1ec3cbcdcc9ed83ad4f6e72f618a5a3f2b0156266a8ae9e"
    assert len(hm.TAG) == 15 == len(b"kosk-regtree-v1") == len(b"kosk-regsort-v1")
    # the three formats share no hash
    assert len({hm.node(ZERO, ONES), tm.node(ZERO, ONES), sm.node(ZERO, ONES)}) == 3 and hm.empty(2) not in (tm.EMPTY[2], sm.PAD[2])
    # the stored record and its leaf
    assert hm.leaf(3, hm.record(hm.ADMIT, 0)).hex() == hm.PINS["V"] and hm.leaf(3, hm.record(hm.CHECKPOINT, 0, 1, ZERO, ONES)).hex() == hm.PINS["C"]
    # the tree of three leaves, by hand
    a, b, c = (bytes([i]) * 32 for i in (1, 2, 3))
    assert hm.mth(2, [a, b, c]) == hm.node(hm.node(a, b), c) and hm.path(2, 2, [a, b, c]) == [hm.node(a, b)] and hm.path(2, 0, [a, b, c]) == [b, c]
    assert hm.proof(2, 2, [a, b, c]) == [c] and hm.proof(2, 1, [a, b, c]) == [b, c] and hm.proof(2, 3, [a, b, c]) == [] == hm.proof(2, 0, [a, b, c])


def test_names_are_declared_bound_and_exported(api):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in HOST + HANDLE:
        assert re.search(r"\b(?:int|size_t) %s\s*\(" % name, code), name
        assert name in api.EXPORTS and hasattr(api.lib, name), name
        assert getattr(api.lib, name).argtypes is not None, name
    for method in METHODS:
        assert callable(getattr(api.Kosk, method)), method
    for fn in FUNCTIONS:
        assert callable(getattr(api, fn)), fn
    for line in ("int kosk_reghist_depth(int size);", "size_t kosk_reghist_path_bytes(int size);", "size_t kosk_reghist_consistency_bytes(int size);",
                 "int kosk_reghist_leaf(int kyber_k, const uint8_t event[80], uint8_t out[32]);",
                 "int kosk_reghist_node(const uint8_t l[32], const uint8_t r[32], uint8_t out[32]);",
                 "int kosk_reghist_empty_root(int kyber_k, uint8_t out[32]);",
                 "int kosk_reghist_root_from_path(int index, int size, const uint8_t leaf[32], const uint8_t *record, uint8_t root[32]);",
                 "int kosk_reghist_check_consistency(int old_size, int size, const uint8_t root_old[32], const uint8_t root_new[32], const uint8_t *record);",
                 "int kosk_registry_history_reserve(kosk_ctx *ctx, int max_events);",
                 "int kosk_registry_history_level(const kosk_ctx *ctx, int *size, int *max_events);",
                 "int kosk_registry_history_head(kosk_ctx *ctx, int size, uint8_t root[32], int *size_out);",
                 "int kosk_registry_history_checkpoint(kosk_ctx *ctx, int *index);",
                 "int kosk_registry_history_read(kosk_ctx *ctx, int first, int n, uint8_t *events);",
                 "int kosk_registry_history_prove_events(kosk_ctx *ctx, int size, int n, const int32_t *index, uint8_t *leaves, uint8_t *records, uint8_t *root);",
                 "int kosk_registry_history_prove_consistency(kosk_ctx *ctx, int size, int n, const int32_t *old_size, uint8_t *records, uint8_t *root);",
                 "enum { KOSK_REGHIST_ADMIT = 1, KOSK_REGHIST_EVICT = 2, KOSK_REGHIST_CHECKPOINT = 3 };", "#define KOSK_REGHIST_EVENT_BYTES 80"):
        assert line in code, line
    m = re.search(r"enum \{ KOSK_REGHIST_TIER_LEVELS = (\d+) \};", code)
    assert m and int(m.group(1)) == api.REGHIST_TIER_LEVELS
    assert (api.REGHIST_ADMIT, api.REGHIST_EVICT, api.REGHIST_CHECKPOINT) == (hm.ADMIT, hm.EVICT, hm.CHECKPOINT) == (1, 2, 3)
    assert api.REGHIST_EVENT_BYTES == hm.EVENT_BYTES == 80


def test_path_ids_and_the_header_sentences(api):
    K = api.Kosk
    assert (K.PATH_REGHIST_APPEND, K.PATH_REGHIST_GROUPS, K.PATH_REGHIST_FRONTIER, K.PATH_REGHIST_PROVE) == (38, 39, 40, 41)
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int kosk_path_count\(", _header(), flags=re.S)
    assert m
    text = re.sub(r"\s*\n \* ", " ", m.group(1))
    assert "38 launches of k_reghist_append (one per tier of an append to the registry history)" in text
    assert "39 leaf groups hashed by those launches" in text
    assert "40 launches of k_reghist_frontier" in text and "a second call at the same size launches nothing" in text
    assert "41 launches of k_reghist_prove (one per launch group of kosk_registry_history_prove_events / _prove_consistency" in text
    assert "ids 27..37 do not move for kosk_registry_history_head, _read or the proving calls" in text
    # the earlier sentences are still there, word for word
    assert "36 launches of k_regsort_tree (one per tier of a rebuild of the sorted tree" in text
    assert "37 launches of k_regsort_prove (one per launch group of kosk_registry_prove_absent)" in text


def test_the_size_functions(api):
    for n in list(range(0, 300)) + [2 ** 10 - 1, 2 ** 10, 2 ** 10 + 1, 2 ** 24, 2 ** 24 + 1, 2 ** 31 - 1]:
        d = 0 if n <= 1 else (n - 1).bit_length()
        assert api.reghist_depth(n) == d == hm.depth(n), n
        assert api.reghist_path_bytes(n) == (16 + 32 * d if n >= 1 else 0) == hm.path_bytes(n), n
        assert api.reghist_consistency_bytes(n) == (16 + 32 * (d + 1) if n >= 1 else 0) == hm.consistency_bytes(n), n
    for n in (-1, -2 ** 31):
        assert api.reghist_depth(n) == -1 and api.reghist_path_bytes(n) == 0 == api.reghist_consistency_bytes(n)


def test_leaf_node_and_empty_root_against_the_model(api):
    rng = random.Random(20370)
    for i in range(300):
        k = 2 + i % 3
        x, y, l, r = (rng.randbytes(32) for _ in range(4))
        a = (0, 1, 2 ** 32 - 1)[i] if i < 3 else rng.randrange(2 ** 32)
        b = rng.randrange(2 ** 32)
        for op in (hm.ADMIT, hm.EVICT):
            assert api.reghist_leaf(k, api.reghist_event(op, a, 0, x)) == hm.event_leaf(k, x, op, a) == hm.leaf(k, hm.record(op, a, 0, x)), i
        assert api.reghist_leaf(k, api.reghist_event(hm.CHECKPOINT, a, b, x, y)) == hm.checkpoint_leaf(k, x, y, a, b), i
        assert api.reghist_node(l, r) == hm.node(l, r), i
        assert api.reghist_event(3, a, b, x, y) == hm.record(3, a, b, x, y)
    for k in (2, 3, 4):
        assert api.reghist_empty_root(k) == hm.empty(k)
    assert api.reghist_leaf(3, hm.record(hm.ADMIT, 0)).hex() == hm.PINS["V"]
    assert api.reghist_leaf(3, hm.record(hm.CHECKPOINT, 0, 1, ZERO, ONES)).hex() == hm.PINS["C"]
    assert api.reghist_node(ZERO, ONES).hex() == hm.PINS["N"]


def test_root_from_path_against_the_model_for_every_leaf_and_size(api, leaves):
    for n in range(1, NMAX + 1):
        root = hm.mth(2, leaves[:n])
        for i in range(n):
            rec = hm.inclusion_record(2, i, leaves[:n])
            assert len(rec) == api.reghist_path_bytes(n)
            assert api.reghist_root_from_path(i, n, leaves[i], rec) == root, (i, n)


def test_check_consistency_against_the_model_for_every_pair(api, leaves):
    roots = [hm.mth(2, leaves[:n]) for n in range(NMAX + 1)]
    for n in range(1, NMAX + 1):
        for m in range(0, n + 1):
            rec = hm.consistency_record(2, m, leaves[:n])
            assert len(rec) == api.reghist_consistency_bytes(n)
            assert api.reghist_check_consistency(m, n, roots[m], roots[n], rec) is True, (m, n)


def _edit(rec, at, value):
    return rec[:at] + value + rec[at + len(value):]


@pytest.mark.parametrize("n", (1, 2, 3, 5, 8, 13, 21, 64, 70))
def test_root_from_path_on_every_rule(n, api, leaves):
    d, root = hm.depth(n), hm.mth(2, leaves[:n])
    for i in range(n):
        p = hm.path(2, i, leaves[:n])
        rec = hm.pack(p, i, n, d)
        assert api.reghist_root_from_path(i, n, leaves[i], rec) == root
        # a record too few, a record too many, a count above the bound
        if p:
            assert api.reghist_root_from_path(i, n, leaves[i], hm.pack(p[:-1], i, n, d)) != root
        if len(p) < d:
            assert api.reghist_root_from_path(i, n, leaves[i], hm.pack(p + [leaves[0]], i, n, d)) is None
            # non-zero padding: the first and the last byte behind the records
            for at in (16 + 32 * len(p), len(rec) - 1):
                assert api.reghist_root_from_path(i, n, leaves[i], _edit(rec, at, b"\x01")) is None
        assert api.reghist_root_from_path(i, n, leaves[i], _edit(rec, 0, struct.pack("<I", d + 1))) is None
        # one altered record, each of them
        for c in range(len(p)):
            assert api.reghist_root_from_path(i, n, leaves[i], _edit(rec, 16 + 32 * c + 31, bytes([rec[16 + 32 * c + 31] ^ 0x80]))) not in (root, None)
        # each header word against the arguments
        assert api.reghist_root_from_path(i, n, leaves[i], _edit(rec, 4, struct.pack("<I", i + 1))) is None
        assert api.reghist_root_from_path(i, n, leaves[i], _edit(rec, 8, struct.pack("<I", n + 1))) is None
        assert api.reghist_root_from_path(i, n, leaves[i], _edit(rec, 12, struct.pack("<I", 1))) is None
        # a wrong index with a header that agrees with it, another leaf
        if n > 1:
            j = (i + 1) % n
            assert api.reghist_root_from_path(j, n, leaves[i], _edit(rec, 4, struct.pack("<I", j))) != root
            assert api.reghist_root_from_path(i, n, leaves[j], rec) != root


@pytest.mark.parametrize("n", (1, 2, 3, 5, 8, 13, 21, 64, 70))
def test_check_consistency_on_every_rule(n, api, leaves):
    d, root = hm.depth(n), hm.mth(2, leaves[:n])
    chk = api.reghist_check_consistency
    for m in range(0, n + 1):
        old = hm.mth(2, leaves[:m])
        p = hm.proof(2, m, leaves[:n])
        rec = hm.pack(p, m, n, d + 1)
        assert chk(m, n, old, root, rec) is True
        if m == 0:
            assert chk(0, n, None, root, rec) is True and chk(0, n, ONES, root, rec) is True  # root_old is not read
            assert chk(0, n, old, root, hm.pack([root], 0, n, d + 1)) is False                 # consistent iff no record
        elif m == n:
            assert chk(n, n, ONES, root, rec) is False and chk(n, n, old, ONES, rec) is False  # the roots are equal
            assert chk(n, n, old, root, hm.pack([root], n, n, d + 1)) is False
        else:
            assert p and chk(m, n, old, root, hm.pack(p[:-1], m, n, d + 1)) is False           # a record too few
            if len(p) < d + 1:
                assert chk(m, n, old, root, hm.pack(p + [p[-1]], m, n, d + 1)) is False        # a record too many
            for c in range(len(p)):                                                            # one altered record
                assert chk(m, n, old, root, _edit(rec, 16 + 32 * c, bytes([rec[16 + 32 * c] ^ 1]))) is False
            assert chk(m, n, ONES, root, rec) is False and chk(m, n, old, ONES, rec) is False
            # a forked old root: the first m leaves with one of them changed
            fork = list(leaves[:m])
            fork[m // 2] = ZERO
            assert chk(m, n, hm.mth(2, fork), root, rec) is False
            # the proof for another old size under this one's header
            if m + 1 < n:
                assert chk(m, n, old, root, hm.pack(hm.proof(2, m + 1, leaves[:n]), m, n, d + 1)) is False
        # the header, the bound, the padding
        assert chk(m, n, old, root, _edit(rec, 4, struct.pack("<I", m + 1))) is False
        assert chk(m, n, old, root, _edit(rec, 8, struct.pack("<I", n + 1))) is False
        assert chk(m, n, old, root, _edit(rec, 12, struct.pack("<I", 1))) is False
        assert chk(m, n, old, root, _edit(rec, 0, struct.pack("<I", d + 2))) is False
        if len(p) < d + 1:
            for at in (16 + 32 * len(p), len(rec) - 1):
                assert chk(m, n, old, root, _edit(rec, at, b"\x01")) is False
    # m > n
    with pytest.raises(api.KoskError):
        chk(n + 1, n, root, root, hm.pack([], n + 1, n, d + 1))
    assert api.lib.kosk_reghist_check_consistency(n + 1, n, root, root, hm.pack([], n + 1, n, d + 1)) == -1


def test_refusals_of_the_host_functions(api):
    lib = api.lib
    a, out = C.create_string_buffer(32), C.create_string_buffer(32)
    leaf, node, empty, rfp, chk = lib.kosk_reghist_leaf, lib.kosk_reghist_node, lib.kosk_reghist_empty_root, lib.kosk_reghist_root_from_path, lib.kosk_reghist_check_consistency
    ev = hm.record(hm.ADMIT, 7, 0, ONES)
    assert leaf(2, ev, out) == 0 and out.raw == hm.event_leaf(2, ONES, 1, 7)
    assert leaf(1, ev, out) == -1 and leaf(5, ev, out) == -1 and leaf(2, None, out) == -1 and leaf(2, ev, None) == -1
    for op in (0, 4, 2 ** 31, 2 ** 32 - 1):                                              # op outside 1..3
        assert leaf(2, hm.record(op, 7, 0, ONES), out) == -1, op
    for bad in (hm.record(1, 7, 1, ONES), hm.record(2, 7, 2 ** 31, ONES), hm.record(1, 7, 0, ONES, b"\x01" + bytes(31)), hm.record(2, 7, 0, ONES, bytes(31) + b"\x80"),
                ev[:12] + b"\x01" + ev[13:], ev[:15] + b"\x80" + ev[16:]):               # b, y and word 12 of ops 1 / 2
        assert leaf(2, bad, out) == -1 and hm.leaf(2, bad) is None
    cp = hm.record(hm.CHECKPOINT, 1, 2, ZERO, ONES)
    assert leaf(2, cp, out) == 0 and leaf(2, cp[:12] + b"\x01" + cp[13:], out) == -1     # word 12 of op 3
    assert node(None, a, out) == -1 and node(a, None, out) == -1 and node(a, a, None) == -1
    assert empty(1, out) == -1 and empty(5, out) == -1 and empty(2, None) == -1 and empty(2, out) == 0 and out.raw == hm.empty(2)
    rec = hm.pack([], 0, 1, 1)
    assert rfp(0, 1, a, rec, out) == 0 and out.raw == a.raw
    assert rfp(0, 0, a, rec, out) == -1 and rfp(-1, 1, a, rec, out) == -1 and rfp(1, 1, a, rec, out) == -1 and rfp(0, -1, a, rec, out) == -1
    assert rfp(0, 1, None, rec, out) == -1 and rfp(0, 1, a, None, out) == -1 and rfp(0, 1, a, rec, None) == -1
    assert chk(0, 1, None, a, rec) == 1 and chk(-1, 1, a, a, rec) == -1 and chk(2, 1, a, a, rec) == -1 and chk(0, 0, a, a, rec) == -1 and chk(0, -1, a, a, rec) == -1
    assert chk(1, 1, None, a, rec) == -1 and chk(0, 1, a, None, rec) == -1 and chk(0, 1, a, a, None) == -1
    # the handle calls without a handle
    i = C.c_int()
    assert lib.kosk_registry_history_reserve(None, 1) == -1 and lib.kosk_registry_history_level(None, C.byref(i), C.byref(i)) == -1
    assert lib.kosk_registry_history_head(None, -1, out, C.byref(i)) == -1 and lib.kosk_registry_history_checkpoint(None, C.byref(i)) == -1
    assert lib.kosk_registry_history_read(None, 0, 1, out) == -1
    q = (C.c_int32 * 1)(0)
    assert lib.kosk_registry_history_prove_events(None, -1, 1, q, out, out, out) == -1
    assert lib.kosk_registry_history_prove_consistency(None, -1, 1, q, out, out) == -1
    with pytest.raises(api.KoskError):
        api.reghist_leaf(5, ev)
    with pytest.raises(api.KoskError):
        api.reghist_leaf(2, ev[:79])
    with pytest.raises(api.KoskError):
        api.reghist_empty_root(1)
    with pytest.raises(api.KoskError):
        api.reghist_root_from_path(0, 2, ZERO, bytes(api.reghist_path_bytes(2) - 1))
    with pytest.raises(api.KoskError):
        api.reghist_check_consistency(0, 2, ZERO, ZERO, bytes(api.reghist_consistency_bytes(2) + 1))
    assert api.reghist_root_from_path(2, 2, ZERO, hm.pack([ZERO], 2, 2, 1)) is None


def test_the_example_parses():
    """examples/registry_history.cpp against the header, host side only"""
    cxx = shutil.which("hipcc") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    cmd = [cxx, "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "registry_history.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout


def test_reghist_host_check(tmp_path):
    """the host source under ASan + UBSan in a stand-alone program: every path and proof up to 40 events from the recursive definition,
    every rule of both verifiers, the refusals"""
    exe = str(tmp_path / "reghist_host_check")
    r = subprocess.run(["c++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "mpcith_kyber_kosk_amd", "csrc"), os.path.join(ROOT, "tests", "reghist_host_check.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    m = re.search(r"reghist checks (\d+) failures 0\n", r.stdout)
    assert r.returncode == 0 and m and int(m.group(1)) >= 1000 and "FAILED" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
