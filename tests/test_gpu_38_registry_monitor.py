"""GPU tests of the registry monitor (include/kosk_mi355x.h: kosk_monitor_reserve / _level / _feed / _head / _roots / _read; INTEGRATION.md
8.8) against the sequential replay of tests/registry_monitor_model.py, the recursive history model of tests/registry_history_model.py and,
on one handle, a registry with a history.  Every comparison is exact."""
import hashlib
import os
import random
import struct
import subprocess

import pytest

from tests import registry_history_model as hm
from tests import registry_monitor_cases as mc
from tests import registry_monitor_model as mm

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
CHUNK = 16384  # KEM_CHUNK: events per launch group
TILE = 2048    # records per LDS tile of the sort
G = 1024       # leaves per group of the history's tier 0
ZERO = bytes(32)


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return torch


@pytest.fixture(scope="module")
def api(torch_cuda):
    from mpcith_kyber_kosk_amd import api
    return api


@pytest.fixture(scope="module")
def ctx(api):
    """one handle for the tests that need nothing but a monitor: every test reserves its own"""
    c = api.Kosk(kyber_k=2, max_batch=3)
    yield c
    c.close()


def key(api, k, tag):
    """any bytes of the right length are a key to kosk_registry_admit"""
    return hashlib.shake_256(b"registry-monitor:%d:" % k + tag).digest(api.pk_bytes(k))


def mon_ids(c):
    return tuple(c.path_count(i) for i in (42, 43, 44, 45))


def heads_of(k, events):
    """the history root at every size 0 .. len(events), each subtree hashed once"""
    leaves = [hm.leaf(k, e) for e in events]
    memo = {}

    def mth(lo, n):
        if n == 0:
            return hm.empty(k)
        if n == 1:
            return leaves[lo]
        got = memo.get((lo, n))
        if got is None:
            s = hm._split(n)
            got = memo[(lo, n)] = hm.node(mth(lo, s), mth(lo + s, n - s))
        return got
    return lambda n: mth(0, n)


def state(c, capacity):
    """everything a monitor reports"""
    return c.monitor_level(), c.monitor_head(), c.monitor_roots(), c.monitor_read(list(range(capacity)))


def check_state(c, k, capacity, max_events, events, failed=False, old_sizes=()):
    """the monitor holds exactly the replay of `events` (a valid log): level, head, both roots, every slot; old heads at old_sizes"""
    ok, _, _, table, n = mm.replay(k, capacity, events)
    assert ok
    head = heads_of(k, events)
    assert c.monitor_level() == (n, max_events, len(table), capacity, failed)
    assert c.monitor_head() == (head(n), n)
    assert c.monitor_roots() == mm.roots(k, capacity, table)
    assert c.monitor_read(list(range(capacity))) == ([int(s in table) for s in range(capacity)], [table.get(s, ZERO) for s in range(capacity)])
    for m in old_sizes:
        assert c.monitor_head(m) == (head(m), m), m


def accepted(c, k, capacity, events, cuts=(), old_sizes=(), spare=0):
    """a fresh monitor fed `events` in the instalments that `cuts` delimit: every feed accepted, then check_state"""
    c.monitor_reserve(capacity, len(events) + spare)
    at = 0
    for cut in list(cuts) + [len(events)]:
        if cut > at:
            assert c.monitor_feed(events[at:cut]) == (True, -1, mm.OK), (at, cut)
            assert c.monitor_level()[0] == cut
        at = cut
    check_state(c, k, capacity, len(events) + spare, events, old_sizes=old_sizes)


def rejected(c, api, k, capacity, events, index, why, cuts=(), what=""):
    """a fresh monitor fed a log with a known first defect: the verdict is the model's and the expected one, then the failed-state
    contract -- failed, size <= bad_index, table, roots and head those of events [0, size), the next feed refused, reserve revives"""
    assert mm.replay(k, capacity, events)[:3] == (False, index, why), what
    c.monitor_reserve(capacity, len(events))
    at, got = 0, None
    for cut in list(cuts) + [len(events)]:
        if cut > at:
            got = c.monitor_feed(events[at:cut])
            if not got[0]:
                break
        at = cut
    assert got == (False, index, why), (what, got, mm.NAMES[why])
    size = c.monitor_level()[0]
    assert size <= index, what
    check_state(c, k, capacity, len(events), events[:size], failed=True)
    with pytest.raises(api.KoskError, match="kosk_monitor_feed: .*failed"):
        c.monitor_feed(events[size:size + 1])
    assert c.monitor_level()[0] == size
    return size


def test_registrar_against_monitor_on_one_handle(api):
    """1. k = 2, 3, 4, capacity 8: admit over occupied slots, evict, enrol, checkpoint, two checkpoints in a row, a checkpoint on the empty
    table; after every call the new events of kosk_registry_history_read are fed and head, roots, table and level compared with the
    registry's, old heads at every earlier size at the end"""
    for k in (2, 3, 4):
        c = api.Kosk(kyber_k=k, max_batch=3)
        keys = [key(api, k, b"one:%d" % i) for i in range(10)]
        cap, mx = 8, 40
        c.registry_reserve(cap)
        c.registry_history_reserve(mx)
        c.monitor_reserve(cap, mx)
        slots = list(range(cap))

        def step(fn):
            fn()
            fed, size = c.monitor_level()[0], c.registry_history_level()[0]
            if size > fed:
                assert c.monitor_feed(c.registry_history_read(fed, size - fed)) == (True, -1, api.MONITOR_OK)
            assert c.monitor_head() == c.registry_history_head()
            assert c.monitor_roots() == (c.registry_root()[0], c.registry_sorted_root()[0])
            states, _, hs = c.registry_read(slots)
            assert c.monitor_read(slots) == (states, hs)
            assert c.monitor_level() == (size, mx) + c.registry_level() + (False,)
        step(lambda: c.registry_admit(keys[:3], [0, 2, 5]))
        step(lambda: c.registry_admit(keys[3:6], [2, 7, 0]))
        step(lambda: c.registry_evict([1, 2, 2, 5]))
        step(lambda: c.registry_enrol(keys[5:8]))
        step(lambda: c.registry_history_checkpoint())
        step(lambda: c.registry_admit(keys[8:9], [6]))
        step(lambda: c.registry_history_checkpoint())
        step(lambda: c.registry_history_checkpoint())
        step(lambda: c.registry_evict(slots))
        step(lambda: c.registry_history_checkpoint())
        size = c.monitor_level()[0]
        assert c.registry_level() == (0, cap) and size >= 20
        for m in range(size + 1):
            assert c.monitor_head(m) == c.registry_history_head(m), m
        events = c.registry_history_read()
        assert mm.replay(k, cap, events) == (True, -1, mm.OK, {}, size)
        c.close()


@pytest.mark.parametrize("capacity", (1, 2, 1025, 2049))
def test_model_made_logs_without_a_registry(ctx, capacity):
    """2. depth 0, one leaf subtree, two and three leaf subtrees: a log fed as one call, and a short one split at every position, with
    identical results"""
    k = 2
    events = mc.random_log(k, capacity, 300, 3800 + capacity, 37)
    accepted(ctx, k, capacity, events, old_sizes=(0, 1, 36, 37, 38, 299))
    short = mc.random_log(k, capacity, 14, 3900 + capacity, 4)
    accepted(ctx, k, capacity, short)
    whole = state(ctx, capacity)
    for cut in range(1, len(short)):
        ctx.monitor_reserve(capacity, len(short))
        assert ctx.monitor_feed(short[:cut]) == (True, -1, mm.OK) and ctx.monitor_feed(b"".join(short[cut:])) == (True, -1, mm.OK)
        assert state(ctx, capacity) == whole, cut


@pytest.mark.parametrize("n", (1, 2, TILE - 1, TILE, TILE + 1, CHUNK, CHUNK + 1))
def test_segment_sizes(ctx, n):
    """3. one segment of n events and the checkpoint behind it in one call: one LDS tile, a tile and the steps in HBM, one and two launch groups"""
    k, capacity = 2, 2049
    events = mc.random_log(k, capacity, n, 38000 + n)
    events = events + [mm.checkpoint(k, capacity, mm.replay(k, capacity, events)[3])]
    before = mon_ids(ctx)
    accepted(ctx, k, capacity, events)
    segments = 2 if n > CHUNK else 1
    leaves = segments + 1  # one tier-0 append per segment and one for the checkpoint
    assert tuple(a - b for a, b in zip(mon_ids(ctx), before)) == (segments, 2 * segments, leaves, 1)


def test_chains(ctx):
    """3. a slot's chain that crosses the group boundary; one slot admitted and evicted 1 000 times in one segment; a segment that touches
    every slot of capacity 2 049 once, in a shuffled order"""
    k, capacity = 2, 2049
    front = mc.random_log(k, capacity, CHUNK - 2, 38100, lo=1)
    chain = []
    for i in range(3):
        chain += [hm.record(hm.ADMIT, 0, 0, mc.fp(b"chain:%d" % i)), hm.record(hm.EVICT, 0, 0, mc.fp(b"chain:%d" % i))]
    events = front + chain[:5]
    events.append(mm.checkpoint(k, capacity, mm.replay(k, capacity, events)[3]))
    accepted(ctx, k, capacity, events)
    assert ctx.monitor_read([0]) == ([1], [mc.fp(b"chain:2")])
    # the last event of the first group admits, the first of the second evicts with the fingerprint of the admission before: it sees the
    # ADMIT in front of the boundary, which the first group committed
    bad = front[:-1] + chain[:3] + [hm.record(hm.EVICT, 0, 0, mc.fp(b"chain:0"))]
    assert len(bad) == CHUNK + 1 and mm.replay(k, capacity, bad)[:3] == (False, CHUNK, mm.EVICT_MISMATCH)
    ctx.monitor_reserve(capacity, len(bad))
    assert ctx.monitor_feed(bad) == (False, CHUNK, mm.EVICT_MISMATCH)
    assert ctx.monitor_level()[0] == CHUNK and ctx.monitor_read([0]) == ([1], [mc.fp(b"chain:1")])
    many = mc.fill(k, capacity, [7, 3, 9])
    for i in range(1000):
        many += [hm.record(hm.EVICT, 3, 0, mc.fp(b"fill:3" if i == 0 else b"many:%d" % (i - 1))), hm.record(hm.ADMIT, 3, 0, mc.fp(b"many:%d" % i))]
    many.append(mm.checkpoint(k, capacity, mm.replay(k, capacity, many)[3]))
    accepted(ctx, k, capacity, many)
    order = list(range(capacity))
    random.Random(381).shuffle(order)
    every = mc.fill(k, capacity, order)
    every.append(mm.checkpoint(k, capacity, mm.replay(k, capacity, every)[3]))
    accepted(ctx, k, capacity, every)
    assert ctx.monitor_level()[2] == capacity


def test_history_edges(ctx):
    """4. feeds that end at sizes 1 023, 1 024 and 1 025, one feed that crosses three leaf groups, old heads on both sides of every
    boundary; a checkpoint as the very first event"""
    k, capacity = 2, 5
    events = mc.random_log(k, capacity, 3 * G + 100, 384, 97)
    edges = [G - 1, G, G + 1, G + 50]
    accepted(ctx, k, capacity, events, cuts=edges, old_sizes=[0, 1, G - 1, G, G + 1, 2 * G - 1, 2 * G, 2 * G + 1, 3 * G, 3 * G + 99])
    first = [mm.checkpoint(k, capacity, {})] + mc.fill(k, capacity, [4, 0])
    accepted(ctx, k, capacity, first, old_sizes=(0, 1, 2))
    assert first[0][:16] == struct.pack("<IIII", 3, 0, capacity, 0)


def test_counters(api, ctx):
    """5. ids 42..45 move as the header says, not for head, roots, read or level; ids 27..41 of a registry on another handle are untouched"""
    k, capacity = 2, 8
    other = api.Kosk(kyber_k=k, max_batch=3)
    other.registry_reserve(4)
    other.registry_history_reserve(8)
    other.registry_admit([key(api, k, b"other")], [1])
    other.registry_history_checkpoint()
    old = tuple(other.path_count(i) for i in range(27, 42))
    events = mc.scripted(k)
    ops = [e[0] for e in events]
    segments = sum(1 for i, op in enumerate(ops) if op != 3 and (i == 0 or ops[i - 1] == 3))
    cps = ops.count(3)
    ctx.monitor_reserve(capacity, len(events))
    before = mon_ids(ctx)
    reused = tuple(ctx.path_count(i) for i in (32, 33, 35, 36, 38, 39, 40))
    assert ctx.monitor_feed(events) == (True, -1, mm.OK)
    after = mon_ids(ctx)
    assert tuple(a - b for a, b in zip(after, before)) == (segments, 2 * segments, segments + cps, cps) == (3, 6, 7, 4)
    moved = tuple(a - b for a, b in zip((ctx.path_count(i) for i in (32, 33, 35, 36, 38, 39, 40)), reused))
    # the slot tree and the sorted tree are rebuilt by the first checkpoint behind a segment: three of the four; every append is one group
    assert moved[0] == 3 and moved[1] == 3 and moved[3] == 3 and moved[2] >= 3 + 3 and moved[4] == 0 and moved[5] == segments + cps and moved[6] == 0
    check_state(ctx, k, capacity, len(events), events, old_sizes=range(len(events)))
    ctx.monitor_level()
    assert mon_ids(ctx) == after
    assert tuple(other.path_count(i) for i in range(27, 42)) == old
    assert tuple(other.path_count(i) for i in (42, 43, 44, 45)) == (0, 0, 0, 0)
    other.close()


def test_every_reason_as_the_sole_defect(api, ctx):
    """6. two segments with a checkpoint behind each: every defect of registry_monitor_cases at the first, a middle and the last event of
    each segment and at each checkpoint; all nine reasons occur; a BAD_SLOT of exactly capacity, each reserved field, one flipped bit in
    each checkpoint field are among them"""
    k, capacity = 2, 8
    log = hm.Log(k, capacity)
    log.admit([(0, mc.fp(0)), (2, mc.fp(1)), (5, mc.fp(2)), (7, mc.fp(3))])
    log.evict([2])
    log.admit([(2, mc.fp(4))])
    mc.checkpoint(log)
    log.evict([5])
    log.admit([(1, mc.fp(5)), (5, mc.fp(6)), (0, mc.fp(7))])
    mc.checkpoint(log)
    events = log.events
    ops = [e[0] for e in events]
    assert ops == [1, 1, 1, 1, 2, 1, 3, 2, 2, 1, 1, 1, 3]
    seen = set()
    for i in (0, 3, 5, 7, 9, 11):
        for name, bad, why in mc.mutation_defects(k, capacity, events, i):
            rejected(ctx, api, k, capacity, bad, i, why, what="%d %s" % (i, name))
            seen.add(why)
    for i in (6, 12):
        for name, bad, why in mc.checkpoint_defects(events, i):
            assert rejected(ctx, api, k, capacity, bad, i, why, what="%d %s" % (i, name)) == i  # the segment in front of it is committed
            seen.add(why)
    assert seen == set(range(1, 10))
    # an EVICT whose mismatch is against the table (slot 7, admitted in the segment before the checkpoint) ...
    bad = events[:8] + [hm.record(hm.EVICT, 7, 0, mc.fp(4))] + events[9:]
    rejected(ctx, api, k, capacity, bad, 8, mm.EVICT_MISMATCH, what="against the table")
    rejected(ctx, api, k, capacity, bad, 8, mm.EVICT_MISMATCH, cuts=(7, 8), what="against the table, the segment cut in two calls")
    # ... and one against an earlier ADMIT of the same segment (slot 1, admitted at 9)
    bad = events[:11] + [hm.record(hm.EVICT, 1, 0, mc.fp(6))] + events[12:]
    assert rejected(ctx, api, k, capacity, bad, 11, mm.EVICT_MISMATCH, what="against the segment") == 7
    ctx.monitor_reserve(capacity, 4)  # reserve revives
    assert ctx.monitor_level() == (0, 4, 0, capacity, False) and ctx.monitor_feed(events[:4]) == (True, -1, mm.OK)


def test_two_defects(api, ctx):
    """7. two defects in one segment, the lower index on the higher slot (it sorts later): the lower index is reported; an event with two
    reasons reports the lower code"""
    k, capacity = 2, 8
    base = mc.fill(k, capacity, [6, 1])
    two = base + [hm.record(hm.EVICT, 7, 0, mc.fp(b"x")), hm.record(hm.ADMIT, 1, 0, mc.fp(b"y"))]
    rejected(ctx, api, k, capacity, two, 2, mm.EVICT_EMPTY)
    swapped = base + [hm.record(hm.ADMIT, 6, 0, mc.fp(b"y")), hm.record(hm.EVICT, 0, 0, mc.fp(b"x")), hm.record(hm.ADMIT, 9, 0, mc.fp(b"z"))]
    rejected(ctx, api, k, capacity, swapped, 2, mm.ADMIT_OCCUPIED)
    both = base + [mc.word(mc.flip(hm.record(hm.ADMIT, 1, 0, mc.fp(b"z")), 8), 4, capacity)]
    rejected(ctx, api, k, capacity, both, 2, mm.BAD_RECORD)
    later = base + [hm.record(hm.ADMIT, 6, 0, mc.fp(b"again")), hm.record(hm.EVICT, 6, 0, mc.fp(b"again"))]
    rejected(ctx, api, k, capacity, later, 2, mm.ADMIT_OCCUPIED)


def test_a_defect_in_the_second_launch_group(api, ctx):
    """8. one call of two launch groups, the defect in a segment of the second: everything before that segment is committed, nothing of it"""
    k, capacity = 2, 2049
    events = mc.random_log(k, capacity, CHUNK + 2, 388)
    events.append(mm.checkpoint(k, capacity, mm.replay(k, capacity, events)[3]))
    tail = mc.random_log(k, 2 * capacity, 40, 389, lo=capacity)  # none of these slots exists
    table = mm.replay(k, capacity, events)[3]
    free = [s for s in range(capacity) if s not in table][:6]
    events += mc.fill(k, capacity, free[:3], b"tail") + [tail[0]] + mc.fill(k, capacity, free[3:], b"tail")
    bad = CHUNK + 6
    assert rejected(ctx, api, k, capacity, events, bad, mm.BAD_SLOT) == CHUNK + 3


def test_device_memory_at_odd_offsets(ctx, torch_cuda):
    """9. events and outputs in device memory at odd offsets between 0xA5 sentinels: sentinels intact, results those of the host-memory run"""
    torch = torch_cuda
    k, capacity = 2, 37
    events = mc.random_log(k, capacity, 200, 3890, 41)
    accepted(ctx, k, capacity, events)
    want = state(ctx, capacity)
    blob = b"".join(events)
    d_ev = torch.full((5 + len(blob) + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_ev[5:5 + len(blob)] = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    sizes, offs = (32, 32, 32, 32 * capacity), (1, 3, 7, 9)
    outs = [torch.full((off + sz + 8,), SENTINEL, dtype=torch.uint8, device="cuda") for off, sz in zip(offs, sizes)]
    torch.cuda.synchronize()
    ptr = [t.data_ptr() + off for t, off in zip(outs, offs)]
    ctx.monitor_reserve(capacity, len(events))
    assert ctx.monitor_feed(d_ev.data_ptr() + 5, n=120) == (True, -1, mm.OK)
    assert ctx.monitor_feed(d_ev.data_ptr() + 5 + 120 * 80, n=80) == (True, -1, mm.OK)
    assert ctx.monitor_head(out=ptr[0])[1] == len(events)
    ctx.monitor_roots(out=(ptr[1], ptr[2]))
    states, _ = ctx.monitor_read(list(range(capacity)), out=ptr[3])
    assert state(ctx, capacity) == want and states == want[3][0]
    got = (want[1][0], want[2][0], want[2][1], b"".join(want[3][1]))
    for t, off, w in zip(outs, offs, got):
        assert bytes(t.cpu().numpy()) == bytes([SENTINEL]) * off + w + bytes([SENTINEL]) * 8
    assert bytes(d_ev.cpu().numpy()) == bytes([SENTINEL]) * 5 + blob + bytes([SENTINEL]) * 8
    # a rejected log from device memory: the same verdict
    name, bad, why = mc.checkpoint_defects(events, 40)[4]
    d_bad = torch.frombuffer(bytearray(b"\x00" + b"".join(bad)), dtype=torch.uint8).cuda()
    ctx.monitor_reserve(capacity, len(events))
    assert ctx.monitor_feed(d_bad.data_ptr() + 1, n=len(bad)) == (False, 40, why) == (False, 40, mm.CP_SLOT_ROOT)
    ctx.monitor_roots(out=(None, ptr[1]))
    ctx.monitor_roots(out=(ptr[2], None))
    torch.cuda.synchronize()
    r = mm.roots(k, capacity, mm.replay(k, capacity, events[:40])[3])
    assert bytes(outs[1].cpu().numpy())[3:35] == r[1] and bytes(outs[2].cpu().numpy())[7:39] == r[0]


def test_refusals(api):
    """10. -1 and a text that begins with the call's name, nothing started: no monitor, bad sizes, "monitor is full" at size + n ==
    max_events + 1 while == max_events is accepted, a size above the current one, a slot outside the table, NULL arguments"""
    import ctypes as C
    k = 2
    c = api.Kosk(kyber_k=k, max_batch=3)
    lib, hd = api.lib, c.handle
    events = mc.fill(k, 4, [0, 1, 2, 3])
    for name, fn in (("feed", lambda: c.monitor_feed(events[:1])), ("head", lambda: c.monitor_head()), ("roots", lambda: c.monitor_roots()),
                     ("read", lambda: c.monitor_read([0]))):
        with pytest.raises(api.KoskError, match="kosk_monitor_%s: .*no monitor is reserved" % name):
            fn()
    assert c.monitor_level() == (0, 0, 0, 0, False) and mon_ids(c) == (0, 0, 0, 0)
    for cap, mx, why in ((-1, 4, "capacity"), (4, -1, "max_events"), (4, 2 ** 24 + 1, "max_events"), (4, 0, "both"), (0, 4, "both")):
        with pytest.raises(api.KoskError, match="kosk_monitor_reserve: .*%s" % why):
            c.monitor_reserve(cap, mx)
    c.monitor_reserve(0, 0)  # nothing to free
    c.monitor_reserve(4, 2 ** 24)
    c.monitor_reserve(4, 3)
    assert c.monitor_feed(events[:1]) == (True, -1, mm.OK)
    before = mon_ids(c)
    with pytest.raises(api.KoskError, match="kosk_monitor_feed: monitor is full"):
        c.monitor_feed(events[1:4])
    assert c.monitor_level() == (1, 3, 1, 4, False) and mon_ids(c) == before
    assert c.monitor_feed(events[1:3]) == (True, -1, mm.OK) and c.monitor_level() == (3, 3, 3, 4, False)
    with pytest.raises(api.KoskError, match="kosk_monitor_feed: monitor is full"):
        c.monitor_feed(events[3:4])
    with pytest.raises(api.KoskError, match="kosk_monitor_head: .*size is above"):
        c.monitor_head(4)
    for bad in (-1, 4):
        with pytest.raises(api.KoskError, match="kosk_monitor_read: .*a slot id outside"):
            c.monitor_read([0, bad])
    buf = C.create_string_buffer(80)
    i = C.c_int()
    q = (C.c_int32 * 1)(0)
    assert lib.kosk_monitor_feed(hd, 0, buf, None, None) == -1 and lib.kosk_monitor_feed(hd, 1, None, None, None) == -1
    assert b"kosk_monitor_feed: invalid argument" in lib.kosk_last_error(hd)
    assert lib.kosk_monitor_head(hd, -1, None, C.byref(i)) == -1 and lib.kosk_monitor_read(hd, 0, q, buf, buf) == -1
    assert lib.kosk_monitor_read(hd, 1, None, buf, buf) == -1 and lib.kosk_monitor_read(hd, 1, q, None, buf) == -1
    assert lib.kosk_monitor_read(hd, 1, q, buf, None) == 0 and buf.raw[0] == 1  # h may be NULL
    assert lib.kosk_monitor_roots(hd, None, None) == 0 and lib.kosk_monitor_level(hd, None, None, None, None, None) == 0
    check_state(c, k, 4, 3, events[:3])
    c.monitor_reserve(0, 0)
    assert c.monitor_level() == (0, 0, 0, 0, False)
    c.close()


def test_inventory_and_erasure(api):
    """11. the monitor's buffers are public entries of the inventory: the scan finds a fed fingerprint, the wipes leave the monitor's
    results unchanged; reserving a registry on the same handle again leaves the monitor intact; (0, 0) frees"""
    k, capacity = 2, 6
    c = api.Kosk(kyber_k=k, max_batch=3)
    events = mc.fill(k, capacity, [4, 1], b"erase")  # fingerprints no other test feeds: fresh HBM may hold what an earlier handle freed
    events.append(mm.checkpoint(k, capacity, mm.replay(k, capacity, events)[3]))
    needle = mc.fp(b"erase:4")
    assert c.secret_scan(needle) == 0
    c.registry_reserve(3)
    c.monitor_reserve(capacity, 8)
    assert c.monitor_feed(events) == (True, -1, mm.OK)
    assert c.secret_scan(needle) >= 1  # the table (and the staged records)
    assert c.secret_scan(hm.leaf(k, events[0])) == 1  # the history's leaf
    want = state(c, capacity)
    c.wipe_secrets()
    assert state(c, capacity) == want
    c.set_wipe(api.WIPE_CALL)
    assert c.monitor_feed([hm.record(hm.EVICT, 1, 0, mc.fp(b"erase:1"))]) == (True, -1, mm.OK)
    c.set_wipe(api.WIPE_OFF)
    check_state(c, k, capacity, 8, events + [hm.record(hm.EVICT, 1, 0, mc.fp(b"erase:1"))])
    want = state(c, capacity)
    c.registry_reserve(5)
    c.registry_reserve(0)
    assert state(c, capacity) == want and c.registry_level() == (0, 0)
    c.monitor_reserve(0, 0)
    assert c.secret_scan(needle) == 0 and c.monitor_level() == (0, 0, 0, 0, False)
    c.close()


def test_children(gpu_child):
    """12. a cohort member as monitor, unmerged, in a fresh child process"""
    out = gpu_child("from tests.gpu_child_registry_monitor import cohort_member as f; f(2)")
    assert "cohort_member ok 2" in out


def test_registry_monitor_example(torch_cuda):
    """12. examples/registry_monitor 3 8 prints only lines ending in "= 1" """
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "registry_monitor")
    if not os.path.exists(exe):
        pytest.fail("examples/registry_monitor missing: run __graft_entry__.build()")
    r = subprocess.run([exe, "3", "8"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 6 and all(ln.endswith("= 1") for ln in lines), r.stdout
    assert lines[-1] == "[result] registry_monitor success = 1"
