"""The registry monitor, the parts that need no GPU: the six names are declared, bound and exported, the exact prototype
lines and the enum, the four path ids and the header's sentences for them, api.MONITOR_* against the header, the sequential model of
tests/registry_monitor_model.py on every log registry_history_model.Log produces and on crafted logs with one known defect, the example
under -fsyntax-only, and the refusals that need no handle."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import pytest

from tests import registry_history_model as hm
from tests import registry_monitor_cases as mc
from tests import registry_monitor_model as mm
from tests import registry_sorted_model as sm
from tests import registry_tree_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kosk_monitor_reserve", "kosk_monitor_level", "kosk_monitor_feed", "kosk_monitor_head", "kosk_monitor_roots", "kosk_monitor_read"]
METHODS = ["monitor_reserve", "monitor_level", "monitor_feed", "monitor_head", "monitor_roots", "monitor_read"]
REASONS = ["OK", "BAD_RECORD", "BAD_SLOT", "ADMIT_OCCUPIED", "EVICT_EMPTY", "EVICT_MISMATCH", "CP_USED", "CP_CAPACITY", "CP_SLOT_ROOT", "CP_SORTED_ROOT"]


@pytest.fixture(scope="module")
def api():
    from mpcith_kyber_kosk_amd import api
    return api


def _header():
    return open(os.path.join(ROOT, "include", "kosk_mi355x.h")).read()


def test_names_are_declared_bound_and_exported(api):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in api.EXPORTS and hasattr(api.lib, name), name
        assert getattr(api.lib, name).argtypes is not None, name
    for method in METHODS:
        assert callable(getattr(api.Kosk, method)), method
    for line in ("enum { KOSK_MONITOR_OK = 0, KOSK_MONITOR_BAD_RECORD = 1, KOSK_MONITOR_BAD_SLOT = 2, KOSK_MONITOR_ADMIT_OCCUPIED = 3, KOSK_MONITOR_EVICT_EMPTY = 4,",
                 "       KOSK_MONITOR_EVICT_MISMATCH = 5, KOSK_MONITOR_CP_USED = 6, KOSK_MONITOR_CP_CAPACITY = 7, KOSK_MONITOR_CP_SLOT_ROOT = 8, KOSK_MONITOR_CP_SORTED_ROOT = 9 };",
                 "int kosk_monitor_reserve(kosk_ctx *ctx, int capacity, int max_events);",
                 "int kosk_monitor_level(const kosk_ctx *ctx, int *size, int *max_events, int *used, int *capacity, int *failed);",
                 "int kosk_monitor_feed(kosk_ctx *ctx, int n, const uint8_t *events, int *bad_index, int *reason);",
                 "int kosk_monitor_head(kosk_ctx *ctx, int size, uint8_t root[32], int *size_out);",
                 "int kosk_monitor_roots(kosk_ctx *ctx, uint8_t slot_root[32], uint8_t sorted_root[32]);",
                 "int kosk_monitor_read(kosk_ctx *ctx, int n, const int32_t *slots, uint8_t *state, uint8_t *h);"):
        assert line + "\n" in code, line


def test_the_reasons_against_the_header(api):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for value, name in enumerate(REASONS):
        m = re.search(r"\bKOSK_MONITOR_%s = (\d+)\b" % name, code)
        assert m and int(m.group(1)) == value == getattr(api, "MONITOR_" + name) == getattr(mm, name), name
    assert mm.NAMES == REASONS


def test_path_ids_and_the_header_sentences(api):
    K = api.Kosk
    assert (K.PATH_MONITOR_KEYS, K.PATH_MONITOR_APPLY, K.PATH_MONITOR_LEAVES, K.PATH_MONITOR_CHECK) == (42, 43, 44, 45)
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int kosk_path_count\(", _header(), flags=re.S)
    assert m
    text = re.sub(r"\s*\n \* ", " ", m.group(1))
    assert "42 launches of k_monitor_keys (one per segment of kosk_monitor_feed)" in text
    assert "43 launches of k_monitor_apply (two per segment: check, then commit)" in text
    assert "44 launches of k_monitor_leaves (one per tier-0 append of the monitor's history)" in text
    assert "45 launches of k_monitor_check (one per checkpoint event fed)" in text
    assert "(32, 33, 35, 36, 38..40) on the monitor's handle" in text
    # the earlier sentences are still there, word for word
    assert "36 launches of k_regsort_tree (one per tier of a rebuild of the sorted tree" in text
    assert "37 launches of k_regsort_prove (one per launch group of kosk_registry_prove_absent)" in text
    assert "38 launches of k_reghist_append (one per tier of an append to the registry history)" in text
    assert "39 leaf groups hashed by those launches" in text
    assert "40 launches of k_reghist_frontier" in text and "a second call at the same size launches nothing" in text
    assert "41 launches of k_reghist_prove (one per launch group of kosk_registry_history_prove_events / _prove_consistency" in text
    assert "ids 27..37 do not move for kosk_registry_history_head, _read or the proving calls" in text


def test_the_models_roots_are_the_tree_models():
    """the model hashes only what differs from an empty tree: the same roots as the full levels of the two tree models"""
    for k, capacity in ((2, 1), (3, 2), (2, 5), (4, 8), (2, 37)):
        for table in ({}, {0: mc.fp(1)}, {capacity - 1: mc.fp(2)}, {s: mc.fp(s % 3) for s in range(0, capacity, 2)}, {s: mc.fp(s) for s in range(capacity)}):
            assert mm.slot_root(k, capacity, table) == tm.root(tm.levels(k, capacity, table)), (k, capacity, sorted(table))
            assert mm.sorted_root(k, capacity, table) == sm.root(sm.levels(k, capacity, table)), (k, capacity, sorted(table))


def test_the_model_accepts_what_the_log_model_produces():
    for k in (2, 3, 4):
        events = mc.scripted(k)
        ops = [struct.unpack("<I", e[:4])[0] for e in events]
        assert ops.count(hm.CHECKPOINT) == 4 and ops[-1] == hm.CHECKPOINT and [a == b == hm.CHECKPOINT for a, b in zip(ops, ops[1:])].count(True) == 1
        assert mm.replay(k, 8, events) == (True, -1, mm.OK, {}, len(events))
        for cut in range(len(events) + 1):  # every prefix, and the rest fed onto its table
            ok, _, _, table, size = mm.replay(k, 8, events[:cut])
            assert ok and size == cut and table == hm.replay(events[:cut])
            assert mm.replay(k, 8, events[cut:], table)[:4] == (True, -1, mm.OK, {})
    for capacity, n, every in ((1, 40, 3), (2, 60, 0), (5, 200, 7), (1025, 300, 64), (2049, 120, 2)):
        events = mc.random_log(2, capacity, n, 380 + capacity, every)
        ok, bad, why, table, size = mm.replay(2, capacity, events)
        assert (ok, bad, why, size) == (True, -1, mm.OK, n) and table == hm.replay(events)
    assert mm.replay(3, 4, [mm.checkpoint(3, 4, {})]) == (True, -1, mm.OK, {}, 1)  # a checkpoint as the very first event


def test_the_model_rejects_each_crafted_log():
    k, capacity = 3, 8
    events = mc.scripted(k)
    ops = [struct.unpack("<I", e[:4])[0] for e in events]
    seen = set()
    for i, op in enumerate(ops):
        crafted = mc.checkpoint_defects(events, i) if op == hm.CHECKPOINT else mc.mutation_defects(k, capacity, events, i)
        for name, bad, why in crafted:
            ok, index, reason, table, size = mm.replay(k, capacity, bad)
            assert (ok, index, reason, size) == (False, i, why, i), (i, name, mm.NAMES[reason])
            assert table == hm.replay(events[:i])
            seen.add(why)
    assert seen == set(range(1, 10))
    # two defects: the lower index wins whatever its slot; an event with two reasons reports the lower code
    base = mc.fill(k, capacity, [6, 1])
    two = base + [hm.record(hm.EVICT, 7, 0, mc.fp(b"x")), hm.record(hm.ADMIT, 1, 0, mc.fp(b"y"))]
    assert mm.replay(k, capacity, two)[:3] == (False, 2, mm.EVICT_EMPTY)
    both = base + [mc.word(mc.flip(hm.record(hm.ADMIT, 1, 0, mc.fp(b"z")), 8), 4, capacity)]
    assert mm.replay(k, capacity, both)[:3] == (False, 2, mm.BAD_RECORD)
    # the state an event sees does not depend on the validity of the event before it: after a rejected ADMIT the index stays the lowest
    assert mm.replay(k, capacity, base + [hm.record(hm.ADMIT, 6, 0, mc.fp(b"again")), hm.record(hm.EVICT, 6, 0, mc.fp(b"again"))])[:3] == (False, 2, mm.ADMIT_OCCUPIED)


def test_the_example_parses():
    """examples/registry_monitor.cpp against the header, host side only"""
    cxx = shutil.which("hipcc") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    cmd = [cxx, "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "registry_monitor.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout


def test_refusals_without_a_handle(api):
    lib = api.lib
    i, out = C.c_int(7), C.create_string_buffer(80)
    slots = (C.c_int32 * 1)(0)
    assert lib.kosk_monitor_reserve(None, 4, 4) == -1
    assert lib.kosk_monitor_level(None, C.byref(i), C.byref(i), C.byref(i), C.byref(i), C.byref(i)) == -1 and i.value == 7
    assert lib.kosk_monitor_feed(None, 1, out, C.byref(i), C.byref(i)) == -1 and i.value == 7
    assert lib.kosk_monitor_head(None, -1, out, C.byref(i)) == -1
    assert lib.kosk_monitor_roots(None, out, out) == -1
    assert lib.kosk_monitor_read(None, 1, slots, out, out) == -1
    assert out.raw == bytes(80)
