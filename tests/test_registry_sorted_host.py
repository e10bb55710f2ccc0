"""The sorted tree, format kosk-regsort-v1, the parts that need no GPU: the eight names are declared, bound and
exported, the three path ids and the header's sentences for them, kosk_regsort_proof_bytes, kosk_regsort_leaf / _node / _root_from_path /
_check_proof against the hashlib model of tests/registry_sorted_model.py, every rule of the verifier, every refusal of the host
functions, the example under -fsyntax-only, and tests/regsort_host_check.cpp, a stand-alone program on the host source built with
ASan + UBSan."""
import ctypes as C
import hashlib
import itertools
import os
import random
import re
import shutil
import struct
import subprocess

import pytest

from tests import registry_sorted_model as sm
from tests import registry_tree_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kosk_regsort_proof_bytes", "kosk_regsort_leaf", "kosk_regsort_node", "kosk_regsort_root_from_path", "kosk_regsort_check_proof",
         "kosk_registry_sorted_root", "kosk_registry_prove_absent", "kosk_regsort_order_device"]
METHODS = ["registry_sorted_root", "registry_prove_absent", "regsort_order"]
FUNCTIONS = ["regsort_proof_bytes", "regsort_leaf", "regsort_node", "regsort_root_from_path", "regsort_check_proof"]
ZERO, ONES = bytes(32), b"\xff" * 32


@pytest.fixture(scope="module")
def api():
    from mpcith_kyber_kosk_amd import api
    return api


def _header():
    return open(os.path.join(ROOT, "include", "kosk_mi355x.h")).read()


def test_the_model_pins_the_four_digests():
    for k in (2, 3, 4):
        assert sm.pad(k) == sm.PAD[k] == hashlib.sha3_256(b"kosk-regsort-v1\x01" + bytes([k, 0, 0, 0])).digest()
    assert sm.PAD[2].hex() == "becb0cab467ebf22bfdba3f689f2f5c073785571975013ed08a36f92fc367cf1"
    assert sm.PAD[3].hex() == "4681eaa29349e1b455d902e2fbfdd7fda743ab7db289ea704dd533faf9186bf2"
    assert sm.PAD[4].hex() == "d8d33b6a86723fba711677b6d1fefe8be3f2fd3fb548179cf20d3b79c35d9ed7"
    assert sm.leaf(3, ZERO, 0) == sm.LEAF_ZERO_K3 == hashlib.sha3_256(b"kosk-regsort-v1\x00" + ZERO + bytes(4) + b"\x03\x00\x00\x00").digest()
    assert sm.LEAF_ZERO_K3.hex() == "0f9fbb3cb7e02ac0ce0b815b6ec6cc29edd6595605393f3b604968eede04d643"
    # the two formats share no hash
    assert sm.PAD[2] != tm.EMPTY[2] and sm.node(ZERO, ONES) != tm.node(ZERO, ONES)


def test_the_model_on_every_small_registry():
    """every occupancy pattern of capacities 1, 2, 3, 5 and 8 with a duplicated key among the contents: 00^32, FF^32, every key and every
    key +- 1 get the right kind, the lowest slot, and a record the model's verifier accepts as that kind"""
    cases = 0
    for capacity in (1, 2, 3, 5, 8):
        hs = [hashlib.sha3_256(b"sorted-model:%d" % (s % 4 if capacity == 8 else s)).digest() for s in range(capacity)]
        d = tm.depth(capacity)
        for bits in itertools.product((0, 1), repeat=capacity):
            content = {s: hs[s] for s in range(capacity) if bits[s]}
            lv = sm.levels(2, capacity, content)
            for x in [ZERO, ONES] + [q for h in content.values() for q in [h] + sm.neighbours(h)]:
                kind, rec = sm.prove(2, capacity, content, x, lv)
                holders = [s for s, h in content.items() if h == x]
                assert kind == (sm.PRESENT if holders else sm.ABSENT) == sm.check(2, d, x, rec, sm.root(lv))
                if holders:
                    assert struct.unpack("<i", rec[4:8])[0] == min(holders)
                cases += 1
    assert cases > 3000


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
    assert re.search(r"size_t kosk_regsort_proof_bytes\(int depth\);", code)
    assert re.search(r"int kosk_regsort_leaf\(int kyber_k, const uint8_t \*h, int32_t slot, uint8_t out\[32\]\);", code)
    assert re.search(r"int kosk_regsort_root_from_path\(int kyber_k, int depth, int32_t pos, const uint8_t \*h, int32_t slot, "
                     r"const uint8_t \*path, uint8_t root\[32\]\);", code)
    assert re.search(r"int kosk_regsort_check_proof\(int kyber_k, int depth, const uint8_t x\[32\], const uint8_t \*record, "
                     r"const uint8_t root\[32\]\);", code)
    assert re.search(r"int kosk_registry_sorted_root\(kosk_ctx \*ctx, uint8_t root\[32\], int \*used, int \*capacity\);", code)
    assert re.search(r"int kosk_registry_prove_absent\(kosk_ctx \*ctx, int n, const uint8_t \*h, uint8_t \*kind, uint8_t \*records, "
                     r"uint8_t \*root\);", code)
    assert re.search(r"int kosk_regsort_order_device\(kosk_ctx \*ctx, int n, const uint8_t \*d_h, const uint8_t \*d_flag, "
                     r"int32_t \*d_order\);", code)
    assert (api.REGSORT_NEITHER, api.REGSORT_ABSENT, api.REGSORT_PRESENT) == (sm.NEITHER, sm.ABSENT, sm.PRESENT) == (0, 1, 2)


def test_path_ids_and_the_header_sentences(api):
    assert (api.Kosk.PATH_REGSORT_SORT, api.Kosk.PATH_REGSORT_TREE, api.Kosk.PATH_REGSORT_PROVE) == (35, 36, 37)
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int kosk_path_count\(", _header(), flags=re.S)
    assert m
    text = re.sub(r"\s*\n \* ", " ", m.group(1))
    assert "35 launches of the sort kernels k_regsort_keys / k_regsort_tile / k_regsort_step" in text
    assert "36 launches of k_regsort_tree (one per tier of a rebuild of the sorted tree" in text
    assert "ids 27..34 do not move for any call of that section" in text
    assert "37 launches of k_regsort_prove (one per launch group of kosk_registry_prove_absent)" in text
    # the earlier sentences are still there, word for word
    assert "32 launches of k_registry_tree (one per tier of a rebuild)" in text and "33 leaf subtrees hashed by those launches" in text
    assert "34 launches of k_registry_path (one per launch group of kosk_registry_prove_slots / kosk_registry_prove_peers)" in text


def test_proof_bytes(api):
    for d in range(32):
        assert api.regsort_proof_bytes(d) == 16 + 64 + 64 * d == sm.proof_bytes(d), d
    for d in (-1, 32, 2 ** 31 - 1, -2 ** 31):
        assert api.regsort_proof_bytes(d) == 0 == sm.proof_bytes(d)


def test_leaf_and_node_against_the_model(api):
    rng = random.Random(20360)
    for i in range(300):
        k = 2 + i % 3
        h, l, r = (rng.randbytes(32) for _ in range(3))
        slot = (0, 1, 2 ** 31 - 1)[i] if i < 3 else rng.randrange(2 ** 31)
        assert api.regsort_leaf(k, h, slot) == sm.leaf(k, h, slot), i
        assert api.regsort_node(l, r) == sm.node(l, r), i
    for k in (2, 3, 4):
        assert api.regsort_leaf(k) == sm.PAD[k] == api.regsort_leaf(k, None, 5)
        assert api.regsort_leaf(k, ZERO, 0) == sm.leaf(k, ZERO, 0) != sm.PAD[k]
    assert api.regsort_leaf(3, ZERO, 0) == sm.LEAF_ZERO_K3


@pytest.mark.parametrize("d", (0, 1, 11, 31))
def test_root_from_path_and_check_proof_against_the_model(d, api):
    """random records of every legal flag pattern and some illegal ones: the library's verdict is the model's; and records whose walks
    do lead to the root, built from the model's hashes alone (a depth of 31 allows no whole tree)"""
    rng = random.Random(36 + d)
    edge = [0, (1 << d) - 1]
    for i in range(60):
        k = 2 + i % 3
        pos = edge[i] if i < 2 else rng.randrange(1 << d)
        h = None if i % 4 == 3 else rng.randbytes(32)
        slot = rng.randrange(2 ** 31)
        p = rng.randbytes(32 * d)
        want = sm.root_from_path(k, d, pos, h, slot, p)
        assert api.regsort_root_from_path(k, d, pos, h, slot, p) == want, (d, i)
        if d:
            flipped = bytearray(p)
            flipped[rng.randrange(len(p))] ^= 1 << rng.randrange(8)
            assert api.regsort_root_from_path(k, d, pos, h, slot, bytes(flipped)) != want
        else:
            assert want == (sm.pad(k) if h is None else sm.leaf(k, h, slot))
        # a PRESENT record around that walk
        if h is not None:
            rec = sm.record(pos, slot, 0, 9, h, ZERO, p, bytes(32 * d))
            assert api.regsort_check_proof(k, d, h, rec, want) == sm.PRESENT == sm.check(k, d, h, rec, want)
            assert api.regsort_check_proof(k, d, h, rec, ZERO) == sm.NEITHER == sm.check(k, d, h, rec, ZERO)
    # random records: nothing leads anywhere, and the two verifiers agree on that for every flag pattern
    for flags in list(range(16)) + [16, 0x80000001, 0x103]:
        x, rt = rng.randbytes(32), rng.randbytes(32)
        rec = struct.pack("<iiiI", rng.randrange(-1, 1 << d), rng.randrange(2 ** 31), rng.randrange(2 ** 31), flags) + rng.randbytes(64 + 64 * d)
        assert api.regsort_check_proof(2, d, x, rec, rt) == sm.check(2, d, x, rec, rt) == sm.NEITHER


def _two_keys():
    """entries a < b at positions 0 and 1 of four, Z behind them"""
    a, b = b"\x40" * 32, b"\x80" * 32
    content = {3: a, 1: b}
    return a, b, content, sm.levels(2, 4, content)


def test_check_proof_on_every_rule(api):
    a, b, content, lv = _two_keys()
    rt = sm.root(lv)

    def both(x, rec, root=rt, d=2):
        got = api.regsort_check_proof(2, d, x, rec, root)
        assert got == sm.check(2, d, x, rec, root)
        return got
    x = b"\x60" * 32
    kind, rec = sm.prove(2, 4, content, x, lv)
    assert kind == sm.ABSENT == both(x, rec) and rec[12] == 7
    # each inequality at equality: the same record does not prove the absence of its own neighbours
    assert both(a, rec) == sm.NEITHER and both(b, rec) == sm.NEITHER
    # outside the gap
    assert both(b"\x3f" * 32, rec) == sm.NEITHER and both(b"\x81" * 32, rec) == sm.NEITHER
    # a key leaf claimed as Z
    assert both(x, rec[:12] + b"\x03" + rec[13:]) == sm.NEITHER
    # Z claimed as a key leaf
    y = b"\x90" * 32
    kind, ry = sm.prove(2, 4, content, y, lv)
    assert kind == sm.ABSENT == both(y, ry) and ry[12] == 3
    assert both(y, ry[:12] + b"\x07" + ry[13:48] + ONES + ry[80:]) == sm.NEITHER
    # without a right record pos_l must be P - 1, without a left record -1
    assert both(y, ry[:12] + b"\x01" + ry[13:]) == sm.NEITHER
    assert both(x, rec[:12] + b"\x06" + rec[13:]) == sm.NEITHER
    # stray flag bits, no record at all, bit2 without bit1, PRESENT with other bits
    for flags in (0, 4, 5, 8, 10, 11, 13, 15, 16 | 7, 0x80000007, 0x107):
        assert both(x, rec[:12] + struct.pack("<I", flags) + rec[16:]) == sm.NEITHER, flags
    # PRESENT, and that record for another fingerprint
    kind, rp = sm.prove(2, 4, content, b, lv)
    assert kind == sm.PRESENT == both(b, rp) and rp[12] == 9 and rp[4:8] == struct.pack("<i", 1)
    assert both(x, rp) == sm.NEITHER and both(a, rp) == sm.NEITHER
    # below the first key: no left record; above the last position of a full tree: no right record
    kind, r0 = sm.prove(2, 4, content, ZERO, lv)
    assert kind == sm.ABSENT == both(ZERO, r0) and r0[:4] == b"\xff" * 4 and r0[12] == 6
    assert both(ZERO, struct.pack("<i", 0) + r0[4:]) == sm.NEITHER  # pos_l != -1 without a left record
    full = {0: a, 1: b}
    lf = sm.levels(2, 2, full)
    kind, rl = sm.prove(2, 2, full, y, lf)
    assert kind == sm.ABSENT == both(y, rl, sm.root(lf), 1) and rl[12] == 1 and rl[:4] == struct.pack("<i", 1)
    # pos_l + 1 == P with a right record claimed
    assert both(y, rl[:12] + b"\x03" + rl[13:], sm.root(lf), 1) == sm.NEITHER
    # pos_l outside [0, P)
    for pos in (2, -2, 2 ** 31 - 1, -2 ** 31):
        assert both(y, struct.pack("<i", pos) + rl[4:], sm.root(lf), 1) == sm.NEITHER
    # a left record whose position is not the one before the right record's: the walks do not lead to the root
    assert both(x, struct.pack("<i", 1) + rec[4:]) == sm.NEITHER
    # one flipped bit in each field, on each of the records above
    for q, r, d, root in ((x, rec, 2, rt), (y, ry, 2, rt), (b, rp, 2, rt), (ZERO, r0, 2, rt), (y, rl, 1, sm.root(lf))):
        flags = r[12]
        fields = [0, 12, 13, 15]
        if flags & 1:
            fields += [4, 7, 16, 47] + [80 + 32 * l for l in range(d)]
        if flags & 4:
            fields += [8, 48, 79]
        if flags & 2:
            fields += [80 + 32 * d + 32 * l + 31 for l in range(d)]
        for at in fields:
            for bit in (0, 7):
                bad = bytearray(r)
                bad[at] ^= 1 << bit
                assert both(q, bytes(bad), root, d) == sm.NEITHER, (q.hex()[:4], at, bit)
        # another k, another root
        assert api.regsort_check_proof(3, d, q, r, root) == sm.NEITHER == both(q, r, ONES, d)


def test_refusals_of_the_host_functions(api):
    lib = api.lib
    a, out, path = C.create_string_buffer(32), C.create_string_buffer(32), C.create_string_buffer(64)
    rec = C.create_string_buffer(sm.proof_bytes(1))
    leaf, node, rfp, chk = lib.kosk_regsort_leaf, lib.kosk_regsort_node, lib.kosk_regsort_root_from_path, lib.kosk_regsort_check_proof
    assert leaf(1, a, 0, out) == -1 and leaf(5, None, 0, out) == -1 and leaf(2, a, 0, None) == -1 and leaf(2, a, -1, out) == -1
    assert leaf(2, None, -1, out) == 0 and out.raw == sm.PAD[2]
    assert node(None, a, out) == -1 and node(a, None, out) == -1 and node(a, a, None) == -1
    assert rfp(1, 1, 0, a, 0, path, out) == -1 and rfp(5, 1, 0, a, 0, path, out) == -1                # bad k
    assert rfp(2, -1, 0, a, 0, path, out) == -1 and rfp(2, 32, 0, a, 0, path, out) == -1              # depth outside 0..31
    assert rfp(2, 1, -1, a, 0, path, out) == -1 and rfp(2, 1, 2, a, 0, path, out) == -1               # pos outside [0, 2^depth)
    assert rfp(2, 0, 1, a, 0, None, out) == -1 and rfp(2, 31, -2 ** 31, a, 0, path, out) == -1
    assert rfp(2, 1, 0, a, -1, path, out) == -1                                                       # a key leaf with slot < 0
    assert rfp(2, 1, 0, a, 0, path, None) == -1 and rfp(2, 1, 0, a, 0, None, out) == -1               # NULL out, NULL path with depth > 0
    assert rfp(2, 0, 0, a, 0, None, out) == 0 and out.raw == sm.leaf(2, ZERO, 0)                      # depth 0 needs no path
    assert rfp(2, 2, 3, None, -1, path, out) == 0 and out.raw == sm.root_from_path(2, 2, 3, None, 0, bytes(64))
    assert chk(1, 1, a, rec, a) == -1 and chk(5, 1, a, rec, a) == -1 and chk(2, -1, a, rec, a) == -1 and chk(2, 32, a, rec, a) == -1
    assert chk(2, 1, None, rec, a) == -1 and chk(2, 1, a, None, a) == -1 and chk(2, 1, a, rec, None) == -1
    assert chk(2, 1, a, rec, a) == 0
    # the handle calls without a handle
    assert lib.kosk_registry_sorted_root(None, out, None, None) == -1
    assert lib.kosk_registry_prove_absent(None, 1, a, a, rec, out) == -1
    assert lib.kosk_regsort_order_device(None, 1, a, a, a) == -1
    with pytest.raises(api.KoskError):
        api.regsort_leaf(5)
    with pytest.raises(api.KoskError):
        api.regsort_leaf(2, ZERO, -1)
    with pytest.raises(api.KoskError):
        api.regsort_root_from_path(2, 2, 4, None, 0, bytes(64))
    with pytest.raises(api.KoskError):
        api.regsort_root_from_path(2, 2, 0, None, 0, bytes(63))
    with pytest.raises(api.KoskError):
        api.regsort_check_proof(2, 2, ZERO, bytes(sm.proof_bytes(2) - 1), ZERO)
    with pytest.raises(api.KoskError):
        api.regsort_check_proof(5, 2, ZERO, bytes(sm.proof_bytes(2)), ZERO)


def test_the_example_parses():
    """examples/registry_absent.cpp against the header, host side only"""
    cxx = shutil.which("hipcc") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    cmd = [cxx, "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "registry_absent.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout


def test_regsort_host_check(tmp_path):
    """the host source under ASan + UBSan in a stand-alone program: every rule of the verifier, paths at depths 0 and 31, the refusals"""
    exe = str(tmp_path / "regsort_host_check")
    r = subprocess.run(["c++", "-std=c++20", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "mpcith_kyber_kosk_amd", "csrc"), os.path.join(ROOT, "tests", "regsort_host_check.cpp"), "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    m = re.search(r"regsort checks (\d+) failures 0\n", r.stdout)
    assert r.returncode == 0 and m and int(m.group(1)) >= 1000 and "FAILED" not in r.stdout and "runtime error" not in r.stdout, r.stdout[-3000:]
