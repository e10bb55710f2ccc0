"""GPU tests of the registry history (include/kosk_mi355x.h: kosk_registry_history_reserve / _level / _head / _checkpoint / _read /
_prove_events / _prove_consistency; INTEGRATION.md 8.7, format kosk-reghist-v1) against the recursive hashlib model of
tests/registry_history_model.py and the host verifiers kosk_reghist_root_from_path / kosk_reghist_check_consistency.  Every comparison is
exact."""
import ctypes as C
import hashlib
import os
import struct
import subprocess

import pytest

from tests import registry_cases as rc
from tests import registry_history_model as hm
from tests import registry_index_model as rm
from tests import registry_sorted_model as sm
from tests import registry_tree_model as tm

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
T = 10  # KOSK_REGHIST_TIER_LEVELS
G = 1 << T
ZERO, ONES = bytes(32), b"\xff" * 32


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return torch


@pytest.fixture(scope="module")
def api(torch_cuda):
    from mpcith_kyber_kosk_amd import api
    assert api.REGHIST_TIER_LEVELS == T
    return api


def key(api, k, tag):
    """any bytes of the right length are a key to kosk_registry_admit"""
    return hashlib.shake_256(b"registry-history:%d:" % k + tag).digest(api.pk_bytes(k))


def hist_ids(ctx):
    return tuple(ctx.path_count(i) for i in (38, 39, 40, 41))


def old_ids(ctx):
    return tuple(ctx.path_count(i) for i in range(27, 38))


class Handle:
    """a handle and the model's log side by side: every mutating call goes to both, then the event list and the head are compared"""

    def __init__(self, api, k, capacity, max_events):
        self.api, self.k = api, k
        self.ctx = api.Kosk(kyber_k=k, max_batch=3)
        self.ctx.registry_reserve(capacity)
        self.ctx.registry_history_reserve(max_events)
        self.log = hm.Log(k, capacity)
        self.max_events = max_events
        self.check(full=True)

    def check(self, full=False):
        n = len(self.log.events)
        assert self.ctx.registry_history_level() == (n, self.max_events)
        if full:
            assert self.ctx.registry_history_read() == self.log.events
        assert self.ctx.registry_history_head() == (hm.mth(self.k, self.log.leaves()), n)

    def admit(self, pks, slots, accept=None, full=True):
        self.ctx.registry_admit(pks, slots, accept)
        self.log.admit([(s, rm.fp(p)) for b, (p, s) in enumerate(zip(pks, slots)) if accept is None or accept[b]])
        self.check(full)

    def evict(self, slots):
        self.ctx.registry_evict(slots)
        self.log.evict(slots)
        self.check(True)

    def enrol(self, pks, accept=None):
        slots, status = self.ctx.registry_enrol(pks, accept)
        self.log.admit([(s, rm.fp(p)) for p, s, st in zip(pks, slots, status) if st == self.api.ENROL_ADMITTED])
        self.check(True)
        return slots, status

    def checkpoint(self):
        index = self.ctx.registry_history_checkpoint()
        content = dict(self.log.table)
        want = self.log.checkpoint(tm.root(tm.levels(self.k, self.log.capacity, content)), sm.root(sm.levels(self.k, self.log.capacity, content)))
        assert index == want
        self.check(True)
        return index

    def close(self):
        self.ctx.close()


def check_proofs(h, sizes, indices=None, olds=None):
    """at each size: the head, inclusion records of `indices` (all below the size by default) and consistency records from `olds` (every
    size up to it by default), byte for byte against the model and through the host verifiers"""
    api, k = h.api, h.k
    for n in sizes:
        leaves = h.log.leaves(n)
        head = hm.mth(k, leaves)
        assert h.ctx.registry_history_head(n) == (head, n)
        idx = [i for i in (range(n) if indices is None else indices) if i < n]
        if idx:
            got_leaves, records, root = h.ctx.registry_history_prove_events(idx, n)
            assert root == head and got_leaves == [leaves[i] for i in idx]
            for i, rec in zip(idx, records):
                assert rec == hm.inclusion_record(k, i, leaves), (i, n)
                assert api.reghist_root_from_path(i, n, leaves[i], rec) == head, (i, n)
        ms = [m for m in (range(n + 1) if olds is None else olds) if m <= n]
        if ms and n:
            records, root = h.ctx.registry_history_prove_consistency(ms, n)
            assert root == head
            for m, rec in zip(ms, records):
                assert rec == hm.consistency_record(k, m, leaves), (m, n)
                assert api.reghist_check_consistency(m, n, hm.mth(k, leaves[:m]), head, rec) is True, (m, n)


def scripted(api, k, short):
    """admit, evict of empty and repeated slots, admit over occupied slots, a masked position, enrol (ADMITTED, DUPLICATE, REJECTED),
    checkpoints between them and on the empty registry at the end"""
    a, b, c, d, e, f, g, x = (key(api, k, b"small:%d" % i) for i in range(8))
    h = Handle(api, k, 3, 40)
    h.admit([a, b], [0, 2])
    h.evict([1, 2, 2])
    h.admit([c, d], [0, 1])
    assert h.checkpoint() == 6
    if not short:
        h.admit([e, f], [2, 1], [1, 0])
        h.evict([1])
        assert h.enrol([c, g, x], [1, 1, 0]) == ([0, 1, -1], [api.ENROL_DUPLICATE, api.ENROL_ADMITTED, api.ENROL_REJECTED])
        h.checkpoint()
        h.evict([0, 1, 2, 0])
        assert h.checkpoint() == 14 and h.log.table == {}
        ops = [struct.unpack("<II", ev[:8]) for ev in h.log.events]
        assert ops == [(1, 0), (1, 2), (2, 2), (2, 0), (1, 0), (1, 1), (3, 2), (1, 2), (2, 1), (1, 1), (3, 3), (2, 0), (2, 1), (2, 2), (3, 0)]
    return h


def test_small_histories(api):
    """1. capacity 3, max_events 40, a scripted sequence with the event list and the head checked after every call; then the heads at every
    size, inclusion proofs of every event at every size above it and consistency proofs for every pair, byte for byte and through the host
    verifiers; ids 27..37 do not move for head, read or the proving calls.  A shorter sequence for k = 3 and 4: the roots differ across k"""
    h = scripted(api, 2, False)
    n = len(h.log.events)
    before = old_ids(h.ctx)
    assert h.ctx.registry_history_head(0) == (hm.empty(2), 0) == (bytes.fromhex(hm.PINS["O2"]), 0)
    check_proofs(h, range(n + 1))
    assert old_ids(h.ctx) == before
    heads = {2: h.ctx.registry_history_head(7)[0]}
    h.close()
    for k in (3, 4):
        h = scripted(api, k, True)
        check_proofs(h, range(len(h.log.events) + 1))
        heads[k] = h.ctx.registry_history_head()[0]
        assert h.ctx.registry_history_head(0)[0] == bytes.fromhex(hm.PINS["O%d" % k])
        h.close()
    assert len(set(heads.values())) == 3


def test_the_event_rule(api):
    """2. within one admitting call the EVICTs come first, then the ADMITs, each in ascending position; replaying kosk_registry_history_read
    reproduces kosk_registry_read of every slot; a checkpoint's record holds exactly kosk_registry_root, kosk_registry_sorted_root, used and
    capacity"""
    k, capacity = 2, 6
    keys = [key(api, k, b"rule:%d" % i) for i in range(9)]
    fps = [rm.fp(p) for p in keys]
    h = Handle(api, k, capacity, 64)
    h.admit(keys[:4], [5, 1, 3, 0])
    h.admit(keys[4:9], [3, 4, 1, 2, 5], [1, 1, 0, 1, 1])
    assert h.ctx.registry_history_read(4) == [hm.record(2, 3, 0, fps[2]), hm.record(2, 5, 0, fps[0]), hm.record(1, 3, 0, fps[4]),
                                              hm.record(1, 4, 0, fps[5]), hm.record(1, 2, 0, fps[7]), hm.record(1, 5, 0, fps[8])]
    h.evict([4, 4, 0])
    index = h.checkpoint()
    events = h.ctx.registry_history_read()
    table = hm.replay(events)
    states, _, hs = h.ctx.registry_read(list(range(capacity)))
    assert states == [int(s in table) for s in range(capacity)] and hs == [table.get(s, ZERO) for s in range(capacity)]
    assert table == h.log.table == {1: fps[1], 2: fps[7], 3: fps[4], 5: fps[8]}
    slot_root, used, cap = h.ctx.registry_root()
    sorted_root = h.ctx.registry_sorted_root()[0]
    assert events[index] == struct.pack("<IIII", 3, used, cap, 0) + slot_root + sorted_root and (used, cap) == (4, capacity)
    h.close()


def test_tier_edges(api):
    """3. sizes that straddle 2^T: one-event appends from 2^T - 1 to 2^T + 1 with the head after each, an append that starts mid-group and
    ends mid-group two groups later, proofs at 2^T - 1, 2^T and 2^T + 1 for the first, last and boundary indices and consistency between
    those sizes; counter 39 moves by ((s + c - 1) >> T) - (s >> T) + 1 per append.  Then one admitting call of 2^T + 5 keys into an empty
    registry: one append across a group boundary"""
    k, long = 2, 2 * G + 52
    total = G + 1 + long
    keys = [key(api, k, b"tier:%d" % i) for i in range(total)]
    h = Handle(api, k, total, total + 7)
    s = 0
    for count in (G - 1, 1, 1, long):
        before = hist_ids(h.ctx)
        h.admit(keys[s:s + count], list(range(s, s + count)), full=False)
        after = hist_ids(h.ctx)
        assert after[1] - before[1] == ((s + count - 1) >> T) - (s >> T) + 1, (s, count)
        assert after[0] - before[0] == (2 if (s + count) >> T > s >> T else 1)  # a second tier iff a level-T node became complete
        s += count
    assert s == total == 3 * G + 53 and ((s - 1) >> T) - ((G + 1) >> T) + 1 == 3
    assert h.ctx.registry_history_read(G - 2, 4) == h.log.events[G - 2:G + 2]
    edge = [0, 1, G - 2, G - 1, G, G + 1]
    sizes = [G - 1, G, G + 1]
    check_proofs(h, sizes, edge, [0, 1] + sizes)
    check_proofs(h, [2 * G, total], edge + [2 * G - 1, 2 * G, total - 1], sizes + [2 * G - 1, 2 * G, total])
    h.close()
    n = G + 5
    h = Handle(api, k, n, n)
    before = hist_ids(h.ctx)
    h.admit(keys[:n], list(range(n - 1, -1, -1)), full=False)
    assert tuple(x - y for x, y in zip(hist_ids(h.ctx), before))[:2] == (2, 2)
    assert h.ctx.registry_history_read() == h.log.events
    check_proofs(h, [n], [0, G - 1, G, n - 1], [G - 1, G, n])
    h.close()


class Ranged:
    """the recursive definition on index ranges of one long leaf list, H(lo, n) = N(H(lo, s), H(lo + s, n - s)), every subtree of 256 leaves
    or more computed once"""

    def __init__(self, k, leaves):
        self.k, self.leaves, self.memo = k, leaves, {}

    def mth(self, lo, n):
        if n == 0:
            return hm.empty(self.k)
        if n == 1:
            return self.leaves[lo]
        got = self.memo.get((lo, n))
        if got is None:
            s = hm._split(n)
            got = hm.node(self.mth(lo, s), self.mth(lo + s, n - s))
            if n >= 256:
                self.memo[(lo, n)] = got
        return got

    def path(self, i, lo, n):
        if n == 1:
            return []
        s = hm._split(n)
        if i < s:
            return self.path(i, lo, s) + [self.mth(lo + s, n - s)]
        return self.path(i - s, lo + s, n - s) + [self.mth(lo, s)]

    def sub(self, m, lo, n, whole):
        if m == n:
            return [] if whole else [self.mth(lo, n)]
        s = hm._split(n)
        if m <= s:
            return self.sub(m, lo, s, whole) + [self.mth(lo + s, n - s)]
        return self.sub(m - s, lo + s, n - s, False) + [self.mth(lo, s)]

    def proof(self, m, n):
        return self.sub(m, 0, n, True) if 0 < m < n else []


def test_ranged_is_the_model():
    leaves = [hashlib.sha3_256(b"ranged:%d" % i).digest() for i in range(41)]
    r = Ranged(2, leaves)
    for n in range(42):
        assert r.mth(0, n) == hm.mth(2, leaves[:n])
        assert all(r.path(i, 0, n) == hm.path(2, i, leaves[:n]) for i in range(n))
        assert all(r.proof(m, n) == hm.proof(2, m, leaves[:n]) for m in range(n + 1))


def test_the_second_tier_edge(api, torch_cuda):
    """4. the history grown past 2^(2T) events with 16 384 keys in device memory admitted over their own slots again and again (an EVICT and
    an ADMIT per key and call): one-event appends from 2^2T - 1 to 2^2T + 1 -- the first completes the node of level 2T and runs three
    tiers --, heads, inclusion and consistency proofs at those sizes and at the end; counters 38 and 39 per append"""
    torch = torch_cuda
    k, C2, E = 2, rc.CHUNK, 1 << (2 * T)
    pkb = api.pk_bytes(k)
    gen = torch.Generator().manual_seed(2037)
    host = torch.randint(0, 256, (C2 * pkb,), dtype=torch.uint8, generator=gen)
    raw = bytes(host.numpy())
    d_keys = host.cuda()
    fps = [hashlib.sha3_256(raw[s * pkb:(s + 1) * pkb]).digest() for s in range(C2)]
    admit = [hm.event_leaf(k, fps[s], hm.ADMIT, s) for s in range(C2)]
    evict = [hm.event_leaf(k, fps[s], hm.EVICT, s) for s in range(C2)]
    rounds = (E - 2 * C2) // (2 * C2)  # 31: the history then holds 2^2T - 16 384 events
    total = E + C2
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(C2)
    ctx.registry_history_reserve(total + 5)
    slots = list(range(C2))

    def appended(fn, s, counts):
        """fn appends len(counts) times, counts[i] events each: ids 38 and 39 move by the tiers and the tier-0 groups of each"""
        before = hist_ids(ctx)
        fn()
        launches = groups = 0
        for c in counts:
            groups += ((s + c - 1) >> T) - (s >> T) + 1
            launches += 1 + sum(1 for t in (1, 2) if (s + c) >> (T * t) > s >> (T * t))
            s += c
        assert ctx.registry_history_level()[0] == s
        assert tuple(x - y for x, y in zip(hist_ids(ctx), before))[:2] == (launches, groups), (s, counts)
        return s

    s = appended(lambda: ctx.registry_admit(d_keys.data_ptr(), slots, n=C2), 0, [C2])
    for _ in range(rounds):
        s = appended(lambda: ctx.registry_admit(d_keys.data_ptr(), slots, n=C2), s, [C2, C2])
    s = appended(lambda: ctx.registry_evict(slots[1:]), s, [C2 - 1])
    assert s == E - 1
    leaves = admit + (evict + admit) * rounds + evict[1:] + evict[:1] + admit[:1] + admit[1:]
    assert len(leaves) == total
    model = Ranged(k, leaves)
    assert ctx.registry_history_head() == (model.mth(0, E - 1), E - 1)
    before = hist_ids(ctx)
    ctx.registry_evict([0])
    assert tuple(x - y for x, y in zip(hist_ids(ctx), before))[:2] == (3, 1) and ctx.registry_history_head() == (model.mth(0, E), E)
    before = hist_ids(ctx)
    ctx.registry_admit(d_keys.data_ptr(), [0], n=1)
    assert tuple(x - y for x, y in zip(hist_ids(ctx), before))[:2] == (1, 1) and ctx.registry_history_head() == (model.mth(0, E + 1), E + 1)
    assert appended(lambda: ctx.registry_admit(d_keys.data_ptr() + pkb, slots[1:], n=C2 - 1), E + 1, [C2 - 1]) == total
    assert ctx.registry_history_read(E - 2, 4) == [hm.record(2, C2 - 1, 0, fps[-1]), hm.record(2, 0, 0, fps[0]), hm.record(1, 0, 0, fps[0]), hm.record(1, 1, 0, fps[1])]
    sizes = [E - 1, E, E + 1, total]
    for n in sizes:
        head = model.mth(0, n)
        assert ctx.registry_history_head(n) == (head, n)
        idx = [i for i in (0, G - 1, G, E - G - 1, E - G, E - 2, E - 1, E, total - 1) if i < n]
        got, records, root = ctx.registry_history_prove_events(idx, n)
        assert root == head and got == [leaves[i] for i in idx]
        for i, rec in zip(idx, records):
            assert rec == hm.pack(model.path(i, 0, n), i, n, hm.depth(n)) and api.reghist_root_from_path(i, n, leaves[i], rec) == head, (i, n)
        olds = [m for m in (0, 1, G, E - G, E - 1, E, E + 1, total) if m <= n]
        records, root = ctx.registry_history_prove_consistency(olds, n)
        assert root == head
        for m, rec in zip(olds, records):
            assert rec == hm.pack(model.proof(m, n), m, n, hm.depth(n) + 1), (m, n)
            assert api.reghist_check_consistency(m, n, model.mth(0, m), head, rec) is True, (m, n)
    ctx.close()


def test_the_frontier_is_cached_per_size(api):
    """a second call at the same size launches no frontier; another size launches one; size 0 never does"""
    k = 2
    h = Handle(api, k, 4, 16)
    h.admit([key(api, k, b"cache:%d" % i) for i in range(3)], [0, 1, 2])
    base = hist_ids(h.ctx)
    h.ctx.registry_history_head()
    h.ctx.registry_history_head(3)
    h.ctx.registry_history_prove_events([0, 2], 3)
    h.ctx.registry_history_prove_consistency([1, 2])
    assert hist_ids(h.ctx) == (base[0], base[1], base[2], base[3] + 2)
    h.ctx.registry_history_head(2)
    h.ctx.registry_history_head(0)
    assert hist_ids(h.ctx) == (base[0], base[1], base[2] + 1, base[3] + 2)
    h.ctx.registry_history_head(3)
    assert hist_ids(h.ctx)[2] == base[2] + 2
    h.close()


def test_buffers_across_a_launch_group(api, torch_cuda):
    """16 385 queries of each kind at size 11: host buffers, and device buffers at odd byte offsets between sentinel bytes; id 41 moves by
    two per call; the events and the head to device memory"""
    torch = torch_cuda
    k, n = 3, rc.CHUNK + 1
    h = Handle(api, k, 5, 16)
    keys = [key(api, k, b"buf:%d" % i) for i in range(8)]
    h.admit(keys[:5], [4, 0, 2, 1, 3])
    h.admit(keys[5:8], [0, 1, 2])
    size = len(h.log.events)
    assert size == 11
    leaves = h.log.leaves()
    head = hm.mth(k, leaves)
    idx = [(b * 7 + b // 41) % size for b in range(n)]
    olds = [(b * 5 + b // 37) % (size + 1) for b in range(n)]
    want_incl = {i: hm.inclusion_record(k, i, leaves) for i in range(size)}
    want_cons = {m: hm.consistency_record(k, m, leaves) for m in range(size + 1)}
    before = hist_ids(h.ctx)
    got_leaves, records, root = h.ctx.registry_history_prove_events(idx)
    assert root == head and got_leaves == [leaves[i] for i in idx] and records == [want_incl[i] for i in idx]
    crecords, root = h.ctx.registry_history_prove_consistency(olds)
    assert root == head and crecords == [want_cons[m] for m in olds]
    assert hist_ids(h.ctx) == (before[0], before[1], before[2], before[3] + 4)  # the frontier of this size ran with the last head
    rec, crec = hm.path_bytes(size), hm.consistency_bytes(size)
    sizes = (32 * n, rec * n, 32, crec * n, 32, 80 * size)
    offs = (3, 1, 5, 7, 9, 11)
    outs = [torch.full((off + sz + 8,), SENTINEL, dtype=torch.uint8, device="cuda") for off, sz in zip(offs, sizes)]
    torch.cuda.synchronize()
    ptr = [t.data_ptr() + off for t, off in zip(outs, offs)]
    h.ctx.registry_history_prove_events(idx, out=tuple(ptr[:3]))
    h.ctx.registry_history_prove_consistency(olds, size, out=tuple(ptr[3:5]))
    h.ctx.registry_history_read(out=ptr[5])
    want = (b"".join(leaves[i] for i in idx), b"".join(want_incl[i] for i in idx), head, b"".join(want_cons[m] for m in olds), head, b"".join(h.log.events))
    for t, off, w in zip(outs, offs, want):
        assert bytes(t.cpu().numpy()) == bytes([SENTINEL]) * off + w + bytes([SENTINEL]) * 8
    d_root = torch.full((1 + 32 + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert h.ctx.registry_history_head(4, out=d_root.data_ptr() + 1)[1] == 4
    assert bytes(d_root.cpu().numpy()) == bytes([SENTINEL]) + hm.mth(k, leaves[:4]) + bytes([SENTINEL]) * 8
    # no leaves and no root at all
    one = C.create_string_buffer(rec)
    q = (C.c_int32 * 1)(9)
    assert api.lib.kosk_registry_history_prove_events(h.ctx.handle, -1, 1, q, None, one, None) == 0 and one.raw == want_incl[9]
    h.close()


def test_refusals(api):
    """-1, a text that begins with the call's name, nothing started or changed: no registry, no history, a registry that is not empty,
    max_events out of range, a second reserve with events, a call whose events do not fit ("history is full"), an index, an old size or
    a size out of range, NULL arguments; the handle still works"""
    k = 2
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    lib, hd = api.lib, ctx.handle
    keys = [key(api, k, b"refuse:%d" % i) for i in range(6)]
    calls = (("reserve", lambda: ctx.registry_history_reserve(4)), ("head", lambda: ctx.registry_history_head()),
             ("checkpoint", lambda: ctx.registry_history_checkpoint()), ("read", lambda: ctx.registry_history_read(0, 1)),
             ("prove_events", lambda: ctx.registry_history_prove_events([0])), ("prove_consistency", lambda: ctx.registry_history_prove_consistency([0])))
    for name, fn in calls:
        with pytest.raises(api.KoskError, match="kosk_registry_history_%s: .*no registry is reserved" % name):
            fn()
    assert ctx.registry_history_level() == (0, 0)
    ctx.registry_reserve(4)
    for name, fn in calls[1:]:
        with pytest.raises(api.KoskError, match="kosk_registry_history_%s: .*no history is reserved" % name):
            fn()
    for bad in (-1, 2 ** 24 + 1):
        with pytest.raises(api.KoskError, match="kosk_registry_history_reserve: .*max_events"):
            ctx.registry_history_reserve(bad)
    ctx.registry_admit(keys[:1], [3])
    with pytest.raises(api.KoskError, match="kosk_registry_history_reserve: .*not empty"):
        ctx.registry_history_reserve(4)
    ctx.registry_evict([3])
    assert hist_ids(ctx) == (0, 0, 0, 0)  # a registry without a history launches none of this
    ctx.registry_history_reserve(8)
    ctx.registry_history_reserve(5)  # allowed again while size == 0
    ctx.registry_admit(keys[:2], [0, 1])
    with pytest.raises(api.KoskError, match="kosk_registry_history_reserve: .*has events"):
        ctx.registry_history_reserve(9)

    def snapshot():
        head = ctx.registry_history_head()  # first: the frontier of a new size runs here, once
        return (head, hist_ids(ctx), old_ids(ctx), ctx.registry_history_level(), ctx.registry_level(), ctx.registry_read([0, 1, 2, 3]))
    base = snapshot()
    assert base[3] == (2, 5)
    # two slots occupied: two keys over them are four events, one over one and two new ones are four
    with pytest.raises(api.KoskError, match="kosk_registry_admit: history is full"):
        ctx.registry_admit(keys[2:4], [0, 1])
    with pytest.raises(api.KoskError, match="kosk_registry_admit: history is full"):
        ctx.registry_admit(keys[2:5], [1, 2, 3])
    full = api.Kosk(kyber_k=k, max_batch=3)
    full.registry_reserve(4)
    full.registry_history_reserve(1)
    with pytest.raises(api.KoskError, match="kosk_registry_enrol: history is full"):
        full.registry_enrol(keys[:2])
    assert full.registry_level() == (0, 4) and full.registry_history_level() == (0, 1) and hist_ids(full) == (0, 0, 0, 0)
    full.close()
    assert snapshot() == base
    for name, fn, why in (("prove_events", lambda: ctx.registry_history_prove_events([0, 2]), "an index outside"),
                          ("prove_events", lambda: ctx.registry_history_prove_events([-1]), "an index outside"),
                          ("prove_events", lambda: ctx.registry_history_prove_events([1], 1), "an index outside"),
                          ("prove_events", lambda: ctx.registry_history_prove_events([0], 3), "size is above"),
                          ("prove_consistency", lambda: ctx.registry_history_prove_consistency([3]), "an old size outside"),
                          ("prove_consistency", lambda: ctx.registry_history_prove_consistency([-1]), "an old size outside"),
                          ("prove_consistency", lambda: ctx.registry_history_prove_consistency([2], 1), "an old size outside"),
                          ("prove_consistency", lambda: ctx.registry_history_prove_consistency([0], 3), "size is above"),
                          ("head", lambda: ctx.registry_history_head(3), "size is above"),
                          ("read", lambda: ctx.registry_history_read(1, 2), "events outside"), ("read", lambda: ctx.registry_history_read(2, 1), "events outside")):
        with pytest.raises(api.KoskError, match="kosk_registry_history_%s: .*%s" % (name, why)):
            fn()
    buf = C.create_string_buffer(512)
    q = (C.c_int32 * 2)(0, 1)
    assert lib.kosk_registry_history_head(hd, -1, None, None) == -1 and b"kosk_registry_history_head: invalid argument" in lib.kosk_last_error(hd)
    assert lib.kosk_registry_history_read(hd, 0, 0, buf) == -1 and lib.kosk_registry_history_read(hd, -1, 1, buf) == -1 and lib.kosk_registry_history_read(hd, 0, 1, None) == -1
    for n in (0, -1):
        assert lib.kosk_registry_history_prove_events(hd, -1, n, q, buf, buf, buf) == -1 and lib.kosk_registry_history_prove_consistency(hd, -1, n, q, buf, buf) == -1
    assert lib.kosk_registry_history_prove_events(hd, -1, 1, None, buf, buf, buf) == -1 and lib.kosk_registry_history_prove_events(hd, -1, 1, q, buf, None, buf) == -1
    assert b"kosk_registry_history_prove_events: invalid argument" in lib.kosk_last_error(hd)
    assert lib.kosk_registry_history_prove_consistency(hd, -1, 1, None, buf, buf) == -1 and lib.kosk_registry_history_prove_consistency(hd, -1, 1, q, None, buf) == -1
    assert snapshot() == base
    # what fits is taken: three more events fill the history, then every appending call is refused and nothing changes
    ctx.registry_evict([1])
    ctx.registry_admit(keys[2:3], [2])
    assert ctx.registry_history_checkpoint() == 4 and ctx.registry_history_level() == (5, 5)
    base = snapshot()
    with pytest.raises(api.KoskError, match="kosk_registry_history_checkpoint: history is full"):
        ctx.registry_history_checkpoint()
    with pytest.raises(api.KoskError, match="kosk_registry_evict: history is full"):
        ctx.registry_evict([0])
    with pytest.raises(api.KoskError, match="kosk_registry_admit: history is full"):
        ctx.registry_admit(keys[3:4], [3])
    ctx.registry_evict([1, 3])  # empty slots: no event, and nothing to refuse
    assert snapshot() == base
    leaves = [hm.leaf(k, e) for e in ctx.registry_history_read()]
    assert ctx.registry_history_head() == (hm.mth(k, leaves), 5)
    ctx.close()


def test_inventory_and_erasure(api):
    """the events, the nodes, the ragged nodes and the staging are public buffers of the inventory; the wipes leave them alone; with a history
    the fingerprint of an evicted key stays in HBM on purpose, without one it is gone; 0 frees the history, and so does a new reserve of
    the registry"""
    k = 2
    pk_a, pk_b = key(api, k, b"erase:a"), key(api, k, b"erase:b")
    fa, fb = rm.fp(pk_a), rm.fp(pk_b)
    h = Handle(api, k, 5, 32)
    ctx = h.ctx
    h.admit([pk_a, pk_b], [1, 3])
    la, lb = hm.event_leaf(k, fa, 1, 1), hm.event_leaf(k, fb, 1, 3)
    head = hm.node(la, lb)
    assert ctx.secret_scan(fa) == 2 and ctx.secret_scan(la) == 1 and ctx.secret_scan(head) >= 1  # the slot and the event; the leaf; the node (and the frontier)
    proved = (ctx.registry_history_prove_events([0, 1]), ctx.registry_history_prove_consistency([0, 1, 2]))
    assert ctx.secret_scan(la) >= 2  # the node and the staged leaf
    ctx.wipe_secrets()
    ctx.set_wipe(api.WIPE_CALL)
    before = hist_ids(ctx)
    assert (ctx.registry_history_prove_events([0, 1]), ctx.registry_history_prove_consistency([0, 1, 2])) == proved
    ctx.set_wipe(api.WIPE_OFF)
    assert hist_ids(ctx) == (before[0], before[1], before[2], before[3] + 2) and ctx.registry_history_read() == h.log.events
    h.evict([1])
    assert ctx.registry_read([1])[2] == [ZERO]
    assert ctx.secret_scan(fa) == 2  # the ADMIT and the EVICT event: a public log remembers
    assert hm.replay(ctx.registry_history_read()) == {3: fb}
    # freeing the history, and a registry without one: the evicted key's fingerprint is gone from HBM
    ctx.registry_history_reserve(0)
    assert ctx.registry_history_level() == (0, 0) and ctx.secret_scan(fa) == 0 and ctx.secret_scan(lb) == 0 and ctx.secret_scan(fb) == 1
    base = hist_ids(ctx)
    ctx.registry_evict([3])
    ctx.registry_admit([pk_a], [0])
    ctx.registry_evict([0])
    assert hist_ids(ctx) == base and ctx.secret_scan(fa) == 0
    # a new reserve of the registry frees the history with everything else
    ctx.registry_history_reserve(8)
    ctx.registry_admit([pk_a], [0])
    ctx.registry_evict([0])
    assert ctx.registry_history_level() == (2, 8) and ctx.secret_scan(fa) == 2
    ctx.registry_reserve(2)
    assert ctx.registry_history_level() == (0, 0) and ctx.secret_scan(fa) == 0
    h.close()


def test_children(gpu_child):
    """a cohort member, unmerged, in a fresh child process; and with KOSK_DEBUG_XOF_BLOCKS=1 an admission that fails with "block limit"
    appends no event"""
    out = gpu_child("from tests.gpu_child_registry_history import cohort_member as f; f(2)")
    assert "cohort_member ok 2" in out
    out = gpu_child("from tests.gpu_child_registry_history import block_limit_appends_nothing as f; f(3)", env={"KOSK_DEBUG_XOF_BLOCKS": "1"})
    assert "block_limit_appends_nothing ok 3" in out


def test_registry_history_example(torch_cuda):
    """examples/registry_history 3 8 prints only lines ending in "= 1" """
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "registry_history")
    if not os.path.exists(exe):
        pytest.fail("examples/registry_history missing: run __graft_entry__.build()")
    r = subprocess.run([exe, "3", "8"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 7 and all(ln.endswith("= 1") for ln in lines), r.stdout
    assert lines[-1] == "[result] registry_history success = 1"
