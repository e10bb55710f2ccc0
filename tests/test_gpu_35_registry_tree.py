"""GPU tests of the registry tree (include/kosk_mi355x.h: kosk_registry_root, kosk_registry_prove_slots, kosk_registry_prove_peers;
INTEGRATION.md 8.5, format kosk-regtree-v1) against the hashlib model of tests/registry_tree_model.py, the fixture keys of
tests/registry_cases.py and the host verifier kosk_regtree_root_from_path.  Every comparison is exact."""
import ctypes as C
import functools
import hashlib
import itertools
import os
import subprocess

import pytest

from tests import kem_fixture as kf
from tests import registry_cases as rc
from tests import registry_index_model as rm
from tests import registry_tree_model as tm

pytestmark = pytest.mark.gpu

KS = rc.KS
SENTINEL = 0xA5


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
def handles(api):
    """one handle per K with the fixture's 130 keys admitted, key i in slot(i) of 300 (D = 9); the tests that change the registry make
    their own"""
    hs = {k: api.Kosk(kyber_k=k, max_batch=3) for k in KS}
    for k, h in hs.items():
        rc.admit_fixture(h, k)
    yield hs
    for h in hs.values():
        h.close()


def key(api, k, tag):
    """any bytes of the right length are a key to kosk_registry_admit"""
    return hashlib.shake_256(b"registry-tree:%d:" % k + tag).digest(api.pk_bytes(k))


def fps(k):
    return [rm.fp(p) for p in rc.pks(k)]


@functools.lru_cache(maxsize=None)
def fixture_levels(k):
    """the model's tree over the fixture registry -- computed once, never modified"""
    return tm.levels(k, rc.CAPACITY, {rc.slot(i): h for i, h in enumerate(fps(k))})


def absent(tag):
    return hashlib.sha3_256(b"registry-tree-absent:%d" % tag).digest()


def tree_ids(ctx, api):
    return tuple(ctx.path_count(i) for i in (api.Kosk.PATH_REGISTRY_TREE, api.Kosk.PATH_REGISTRY_SUBTREES, api.Kosk.PATH_REGISTRY_PATH))


def old_ids(ctx):
    return tuple(ctx.path_count(i) for i in range(27, 32))


def check_tree(ctx, api, k, capacity, content, slots):
    """the root, and for each of `slots` (occupied or not) the state, stored fingerprint and path against the model over
    content = {slot: pk}; every path leads to the root through the host verifier"""
    hs = {s: rm.fp(pk) for s, pk in content.items()}
    lv = tm.levels(k, capacity, hs)
    d = tm.depth(capacity)
    want_root = tm.root(lv)
    assert ctx.registry_root() == (want_root, len(content), capacity)
    states, got_h, paths, root = ctx.registry_prove_slots(slots)
    assert root == want_root
    for b, s in enumerate(slots):
        assert states[b] == (1 if s in hs else 0), s
        assert got_h[b] == hs.get(s, bytes(32)), s
        assert paths[b] == tm.path(lv, s) and len(paths[b]) == 32 * d, s
        assert api.regtree_root_from_path(k, d, s, hs.get(s), paths[b]) == want_root, s
        # the opposite claim about the slot does not lead to the root
        assert api.regtree_root_from_path(k, d, s, None if s in hs else bytes(32), paths[b]) != want_root, s
    return want_root


def small_patterns():
    out = []
    for capacity in (1, 2, 3):
        out += [(capacity, bits) for bits in itertools.product((0, 1), repeat=capacity)]
    out += [(5, bits) for bits in ((0, 0, 0, 0, 0), (1, 1, 1, 1, 1), (1, 0, 0, 0, 1), (0, 1, 1, 0, 0), (0, 0, 0, 0, 1))]
    out += [(8, bits) for bits in ((0,) * 8, (1,) * 8, (1, 0, 1, 0, 1, 0, 1, 0), (0, 0, 0, 1, 1, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0, 1))]
    return out


def test_small_trees(api):
    """1. capacities 1, 2, 3 with every occupancy pattern, 5 and 8 with a handful, k = 2: the root, prove_slots of every slot, empty ones
    included, root_from_path of every path; one pattern again for k = 3 and 4 (LE32(kyber_k) enters both leaves)"""
    roots = {}
    again = [(5, (1, 0, 0, 0, 1)), (5, (0, 0, 0, 0, 0))]
    for k, patterns in ((2, small_patterns()), (3, again), (4, again)):
        ctx = api.Kosk(kyber_k=k, max_batch=3)
        for capacity, bits in patterns:
            ctx.registry_reserve(capacity)
            content = {s: key(api, k, b"small:%d" % s) for s in range(capacity) if bits[s]}
            if content:
                ctx.registry_admit(list(content.values()), list(content))
            roots[(k, capacity, bits)] = check_tree(ctx, api, k, capacity, content, list(range(capacity)))
            if content:
                ctx.registry_evict(list(content))
        ctx.close()
    assert roots[(2, 1, (0,))] == tm.EMPTY[2]
    # another k: other leaves, another root -- also for the all-empty tree, where nothing but LE32(kyber_k) differs
    assert len({roots[(k, 5, (1, 0, 0, 0, 1))] for k in KS}) == 3 and len({roots[(k, 5, (0, 0, 0, 0, 0))] for k in KS}) == 3
    # the root does not bind the capacity: 5 and 8 empty slots are the same eight leaves
    assert roots[(2, 5, (0,) * 5)] == roots[(2, 8, (0,) * 8)] != roots[(2, 3, (0,) * 3)]


@pytest.mark.parametrize("capacity", (1024, 1025, 2049))
def test_tier_edges(capacity, api):
    """2. one full block and one tier; two tiers, the second subtree with one real slot; P = 4096 with a subtree of padding only.  Keys at
    the edges of the subtrees and about 40 spread slots; the paths of those slots and of their empty neighbours"""
    k = 2
    edge = [s for s in (0, 1, 1022, 1023, 1024, 2047, 2048) if s < capacity]
    spread = sorted({(s * 977 + 5) % capacity for s in range(40)} - set(edge))
    occupied = edge + spread
    content = {s: key(api, k, b"tier:%d" % s) for s in occupied}
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(capacity)
    ctx.registry_admit(list(content.values()), occupied)
    around = sorted({t for s in occupied for t in (s - 1, s, s + 1) if 0 <= t < capacity} | {capacity - 1})
    before = tree_ids(ctx, api)
    check_tree(ctx, api, k, capacity, content, around)
    d = tm.depth(capacity)
    assert tree_ids(ctx, api) == (before[0] + max(1, -(-d // 10)), before[1] + max(1, (1 << d) >> 10), before[2] + 1)
    ctx.close()


def test_incremental_rebuilds(api):
    """3. capacity 4096 (two tiers, four leaf subtrees): ids (32, 33) per step, the root against the model after each, and at the end
    against a fresh handle that admitted the final content in one call"""
    k, capacity = 2, 4096
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(capacity)
    content = {s: key(api, k, b"inc:%d" % s) for s in (0, 3, 1023, 1024, 2500, 3071, 4095)}
    ctx.registry_admit(list(content.values()), list(content))

    def step(want):
        before = tree_ids(ctx, api)
        root, used, cap = ctx.registry_root()
        after = tree_ids(ctx, api)
        assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == want + (0,)
        assert (root, used, cap) == (tm.root(tm.levels(k, capacity, {s: rm.fp(p) for s, p in content.items()})), len(content), capacity)
        return root
    roots = [step((2, 4))]
    roots.append(step((0, 0)))
    assert roots[0] == roots[1]
    content[1500] = key(api, k, b"inc:1500")
    ctx.registry_admit([content[1500]], [1500])
    roots.append(step((2, 1)))
    ctx.registry_evict([0, 4095])
    del content[0], content[4095]
    roots.append(step((2, 2)))
    # evicting empty slots changes nothing and rebuilds nothing
    ctx.registry_evict([0, 7])
    roots.append(step((0, 0)))
    new = [key(api, k, b"inc:new:%d" % i) for i in range(3)]
    slots, status = ctx.registry_enrol(new)
    assert slots == [0, 1, 2] and status == [rm.ADMITTED] * 3
    content.update(dict(zip(slots, new)))
    roots.append(step((2, 1)))
    assert len(set(roots)) == 4
    # a masked position of an admission marks nothing: only slot 2000's subtree is rehashed
    content[2000] = key(api, k, b"inc:2000")
    ctx.registry_admit([key(api, k, b"inc:masked"), content[2000]], [3500, 2000], accept=[0, 1])
    roots.append(step((2, 1)))
    check_tree(ctx, api, k, capacity, content, [0, 1, 2, 3, 4, 1500, 2000, 3500, 4095])
    fresh = api.Kosk(kyber_k=k, max_batch=3)
    fresh.registry_reserve(capacity)
    fresh.registry_admit(list(content.values()), list(content))
    assert fresh.registry_root() == (roots[-1], len(content), capacity) and tree_ids(fresh, api) == (2, 4, 0)
    fresh.close()
    ctx.close()


def test_duplicates(api):
    """4. one key in slots 5 and 2 of 8: equal leaves; prove_peers names slot 2; after evicting slot 2 it names slot 5 and the root has
    changed"""
    k = 2
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(8)
    pk, other = rc.pks(k)[7], rc.pks(k)[8]
    h = rm.fp(pk)
    content = {5: pk, 2: pk, 0: other}
    ctx.registry_admit([pk, pk, other], [5, 2, 0])
    root = check_tree(ctx, api, k, 8, content, list(range(8)))
    lv = tm.levels(k, 8, {s: rm.fp(p) for s, p in content.items()})
    assert lv[0][5] == lv[0][2] == tm.leaf(k, h)
    assert ctx.registry_prove_peers([h]) == ([2], [tm.path(lv, 2)], [True], root)
    ctx.registry_evict([2])
    del content[2]
    root2 = check_tree(ctx, api, k, 8, content, list(range(8)))
    lv = tm.levels(k, 8, {s: rm.fp(p) for s, p in content.items()})
    assert root2 != root and ctx.registry_prove_peers([h]) == ([5], [tm.path(lv, 5)], [True], root2)
    ctx.close()


@pytest.mark.parametrize("n", (1, 63, 64, 65, 130))
@pytest.mark.parametrize("k", KS)
def test_prove_peers(k, n, handles, api, torch_cuda):
    """5. n queries on the 130 fixture keys at rc.slot(i), every third a miss: against prove_slots and the model; host buffers, and device
    buffers at odd byte offsets between sentinel bytes"""
    torch = torch_cuda
    ctx = handles[k]
    lv = fixture_levels(k)
    d = tm.depth(rc.CAPACITY)
    hs = [absent(b) if b % 3 == 1 else fps(k)[b] for b in range(n)]
    want_slots = [-1 if b % 3 == 1 else rc.slot(b) for b in range(n)]
    want_paths = [bytes(32 * d) if s < 0 else tm.path(lv, s) for s in want_slots]
    slots, paths, done, root = ctx.registry_prove_peers(hs)
    assert slots == want_slots and done == [s >= 0 for s in want_slots] and root == tm.root(lv) and paths == want_paths
    hit = [b for b in range(n) if want_slots[b] >= 0]
    states, got_h, by_slot, root2 = ctx.registry_prove_slots([want_slots[b] for b in hit])
    assert states == [1] * len(hit) and got_h == [hs[b] for b in hit] and by_slot == [paths[b] for b in hit] and root2 == root
    for b in hit:
        assert api.regtree_root_from_path(k, d, slots[b], hs[b], paths[b]) == root
    # device memory of any alignment
    sizes = (4 * n, 32 * d * n, n, 32)
    d_h = torch.frombuffer(bytearray(b"\x00" + b"".join(hs)), dtype=torch.uint8).cuda()
    outs = [torch.full((off + size + 8,), SENTINEL, dtype=torch.uint8, device="cuda") for off, size in zip((3, 1, 5, 7), sizes)]
    torch.cuda.synchronize()
    ctx.registry_prove_peers(d_h.data_ptr() + 1, n=n, out=tuple(t.data_ptr() + off for t, off in zip(outs, (3, 1, 5, 7))))
    raws = []
    for t, off, size in zip(outs, (3, 1, 5, 7), sizes):
        raw = bytes(t.cpu().numpy())
        assert raw[:off] == bytes([SENTINEL]) * off and raw[off + size:] == bytes([SENTINEL]) * 8
        raws.append(raw[off:off + size])
    assert [int.from_bytes(raws[0][4 * b:4 * b + 4], "little", signed=True) for b in range(n)] == want_slots
    assert raws[1] == b"".join(want_paths) and raws[2] == bytes(s >= 0 for s in want_slots) and raws[3] == root
    assert bytes(d_h.cpu().numpy()) == b"\x00" + b"".join(hs)
    # prove_slots into device memory
    outs = [torch.full((off + size + 8,), SENTINEL, dtype=torch.uint8, device="cuda") for off, size in zip((1, 3, 5), (32 * len(hit), 32 * d * len(hit), 32))]
    torch.cuda.synchronize()
    states, _ = ctx.registry_prove_slots([want_slots[b] for b in hit], out=tuple(t.data_ptr() + off for t, off in zip(outs, (1, 3, 5))))
    assert states == [1] * len(hit)
    for t, off, want in zip(outs, (1, 3, 5), (b"".join(hs[b] for b in hit), b"".join(paths[b] for b in hit), root)):
        raw = bytes(t.cpu().numpy())
        assert raw == bytes([SENTINEL]) * off + want + bytes([SENTINEL]) * 8


@pytest.mark.parametrize("n", (rc.CHUNK, rc.CHUNK + 1))
def test_launch_groups(n, handles, api):
    """5. 16 384 and 16 385 items on the 130-key registry, fingerprints modulo 130 with every 97th a miss: id 34 moves by 1 and by 2; the
    first and last item of each group and a sample"""
    k = 3
    ctx = handles[k]
    lv = fixture_levels(k)
    d = tm.depth(rc.CAPACITY)
    groups = 1 if n <= rc.CHUNK else 2
    idx = [b % kf.ITEMS for b in range(n)]
    f = fps(k)
    hs = [absent(b) if b % 97 == 96 else f[idx[b]] for b in range(n)]
    ctx.registry_root()
    ctx.registry_find(f[:1])  # the tree and the index are current from here on
    before = tree_ids(ctx, api), old_ids(ctx)
    slots, paths, done, root = ctx.registry_prove_peers(hs)
    assert tree_ids(ctx, api) == (before[0][0], before[0][1], before[0][2] + groups)
    assert old_ids(ctx) == before[1][:3] + (before[1][3] + groups, before[1][4])
    assert slots == [-1 if b % 97 == 96 else rc.slot(idx[b]) for b in range(n)] and done == [b % 97 != 96 for b in range(n)]
    assert root == tm.root(lv) and len(paths) == n
    probe = sorted({0, 1, 95, 96, 97, rc.CHUNK - 2, rc.CHUNK - 1, n - 1} | set(range(0, n, 1009)))
    assert any(b % 97 == 96 for b in probe)
    for b in probe:
        assert paths[b] == (bytes(32 * d) if b % 97 == 96 else tm.path(lv, rc.slot(idx[b]))), b
    named = [rc.slot(i) for i in idx]
    states, got_h, by_slot, root2 = ctx.registry_prove_slots(named)
    assert tree_ids(ctx, api) == (before[0][0], before[0][1], before[0][2] + 2 * groups) and root2 == root and states == [1] * n
    for b in probe:
        assert by_slot[b] == tm.path(lv, named[b]) and got_h[b] == f[idx[b]], b


def test_refusals(api):
    """6. NULL arguments, n < 1, a slot out of range, no registry: -1, a text that begins with the call's name, counters and level
    unchanged; the handle still works"""
    k = 3
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    lib, h = api.lib, ctx.handle
    pk = rc.pks(k)[0]
    fp = rm.fp(pk)

    def snapshot():
        return rc.counts(ctx, api) + old_ids(ctx) + tree_ids(ctx, api)

    def refused(name, text, fn):
        before = snapshot()
        with pytest.raises(api.KoskError, match="kosk_%s: .*%s" % (name, text)):
            fn()
        assert snapshot() == before
    refused("registry_root", "no registry is reserved", lambda: ctx.registry_root())
    refused("registry_prove_slots", "no registry is reserved", lambda: ctx.registry_prove_slots([0]))
    refused("registry_prove_peers", "no registry is reserved", lambda: ctx.registry_prove_peers([fp]))
    ctx.registry_reserve(4)
    ctx.registry_admit([pk], [1])
    refused("registry_prove_slots", "outside", lambda: ctx.registry_prove_slots([1, 4]))
    refused("registry_prove_slots", "outside", lambda: ctx.registry_prove_slots([-1]))
    before = snapshot()
    slots = (C.c_int32 * 2)(0, 1)
    buf = C.create_string_buffer(256)
    for n in (0, -1):
        assert lib.kosk_registry_prove_slots(h, n, slots, buf, buf, buf, buf) == -1
        assert lib.kosk_registry_prove_peers(h, n, buf, slots, buf, buf, buf) == -1
    assert lib.kosk_registry_root(h, None, None, None) == -1 and b"kosk_registry_root: invalid argument" in lib.kosk_last_error(h)
    assert lib.kosk_registry_prove_slots(h, 1, None, buf, buf, buf, buf) == -1 and b"kosk_registry_prove_slots: invalid argument" in lib.kosk_last_error(h)
    assert lib.kosk_registry_prove_slots(h, 1, slots, None, buf, buf, buf) == -1
    assert lib.kosk_registry_prove_slots(h, 1, slots, buf, buf, None, buf) == -1  # D = 2: paths are required
    assert lib.kosk_registry_prove_peers(h, 1, None, slots, buf, buf, buf) == -1 and b"kosk_registry_prove_peers: invalid argument" in lib.kosk_last_error(h)
    assert lib.kosk_registry_prove_peers(h, 1, buf, None, buf, buf, buf) == -1 and lib.kosk_registry_prove_peers(h, 1, buf, slots, buf, None, buf) == -1
    assert lib.kosk_registry_prove_peers(h, 1, buf, slots, None, buf, buf) == -1
    assert snapshot() == before and tree_ids(ctx, api) == (0, 0, 0)
    # the optional outputs may be NULL, and the handle still works
    state = C.create_string_buffer(2)
    assert lib.kosk_registry_prove_slots(h, 2, slots, state, None, buf, None) == 0 and state.raw == b"\x00\x01"
    lv = tm.levels(k, 4, {1: fp})
    assert buf.raw[:128] == tm.path(lv, 0) + tm.path(lv, 1)
    assert ctx.registry_prove_peers([fp]) == ([1], [tm.path(lv, 1)], [True], tm.root(lv))
    # capacity 1: D = 0, no path bytes at all
    ctx.registry_evict([1])
    ctx.registry_reserve(1)
    ctx.registry_admit([pk], [0])
    state = C.create_string_buffer(1)
    assert lib.kosk_registry_prove_slots(h, 1, slots, state, None, None, buf) == 0 and buf.raw[:32] == tm.leaf(k, fp) and state.raw == b"\x01"
    assert ctx.registry_prove_peers([fp, absent(1)]) == ([0, -1], [b"", b""], [True, False], tm.leaf(k, fp))
    ctx.close()


def test_inventory_and_erasure(api):
    """7. the tree is a public buffer of the inventory from the first tree call on; the wipes leave it alone; after an eviction and the
    next root the evicted key's leaf is gone"""
    k = 2
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(5)
    pk_a, pk_b = rc.pks(k)[3], rc.pks(k)[4]
    fa, fb = rm.fp(pk_a), rm.fp(pk_b)
    ctx.registry_admit([pk_a, pk_b], [1, 3])
    assert ctx.secret_scan(tm.EMPTY[k]) == 0 and ctx.secret_scan(tm.leaf(k, fa)) == 0
    lv = tm.levels(k, 5, {1: fa, 3: fb})
    root = ctx.registry_root()[0]
    assert root == tm.root(lv)
    assert ctx.secret_scan(tm.EMPTY[k]) == 6  # three empty slots and three padding leaves, before any path is staged
    assert ctx.secret_scan(tm.leaf(k, fa)) == 1 and ctx.secret_scan(root) == 1
    proved = ctx.registry_prove_slots([0, 1, 2, 3, 4])
    peers = ctx.registry_prove_peers([fa, fb, absent(0)])
    assert proved[2] == [tm.path(lv, s) for s in range(5)] and peers[:3] == ([1, 3, -1], [tm.path(lv, 1), tm.path(lv, 3), bytes(96)], [True, True, False])
    assert ctx.secret_scan(fa) == 1  # in the slot, and nowhere else: the staged query fingerprints are gone
    built = ctx.path_count(api.Kosk.PATH_REGISTRY_TREE)
    ctx.wipe_secrets()
    assert ctx.registry_root()[0] == root and ctx.registry_prove_slots([0, 1, 2, 3, 4]) == proved
    ctx.set_wipe(api.WIPE_CALL)
    coins = list(rc.messages(k)[3:5])
    enc = ctx.kem_enc_slots([1, 3], coins)
    assert enc[2] == [True, True] and kf.sha3(enc[0][0]) == rc.items(k)[3]["ct"]
    assert ctx.registry_root()[0] == root and ctx.registry_prove_peers([fa, fb, absent(0)]) == peers
    assert ctx.registry_prove_slots([0, 1, 2, 3, 4]) == proved
    ctx.set_wipe(api.WIPE_OFF)
    assert ctx.path_count(api.Kosk.PATH_REGISTRY_TREE) == built == 1
    ctx.registry_evict([1])
    lv2 = tm.levels(k, 5, {3: fb})
    assert ctx.registry_root() == (tm.root(lv2), 1, 5)
    # gone from the tree, and from the staged paths of the earlier tree state (slot 0's path held it): a rebuild clears the staging
    assert ctx.secret_scan(tm.leaf(k, fa)) == 0 and ctx.secret_scan(fa) == 0 and ctx.secret_scan(tm.leaf(k, fb)) == 1
    states, hs, paths, root2 = ctx.registry_prove_slots([1])
    assert states == [0] and hs == [bytes(32)] and api.regtree_root_from_path(k, 3, 1, None, paths[0]) == root2 == tm.root(lv2)
    # reserve drops the tree with the registry
    ctx.registry_evict([3])
    ctx.registry_reserve(2)
    assert ctx.secret_scan(tm.EMPTY[k]) == 0
    assert ctx.registry_root() == (tm.node(tm.EMPTY[k], tm.EMPTY[k]), 0, 2) and ctx.secret_scan(tm.EMPTY[k]) == 2
    ctx.close()


def test_neighbours(api, oracle, gpu_child):
    """8. find, enrol, enc_peers, enc_slots, read and enc_verified return the same bytes before and after the new calls, and ids 27-31
    move only as those calls move them; a cohort member, unmerged, in a fresh child process"""
    k = 3
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    tapes = [oracle.tape_bytes_for(k, 30 + i) for i in range(3)]
    pks, sks, pis = ctx.verifiable_keygen(tapes)
    assert ctx.verify(pis, pks) == [True] * 3
    rc.admit_fixture(ctx, k)
    idx = [0, 97, 24, 2]
    slots = [rc.slot(i) for i in idx]
    coins = [rc.messages(k)[i] for i in idx]
    f = [fps(k)[i] for i in idx]

    def neighbours():
        return [ctx.registry_find(f + [absent(3)]), ctx.registry_enrol([rc.pks(k)[i] for i in idx]), ctx.kem_enc_peers(f, coins),
                ctx.kem_enc_slots(slots, coins), ctx.registry_read(slots + [1]), ctx.kem_enc_verified(3, coins[:3]), ctx.registry_level()]
    start = old_ids(ctx)
    first = neighbours()
    moved = tuple(b - a for a, b in zip(start, old_ids(ctx)))
    assert moved == (0, 1, 1, 3, 1)  # one index build; find, enrol and enc_peers look up; enc_slots and enc_peers encapsulate
    assert first[0] == slots + [-1] and first[1] == (slots, [rm.DUPLICATE] * 4)
    before = old_ids(ctx)
    lv = fixture_levels(k)
    assert ctx.registry_root() == (tm.root(lv), kf.ITEMS, rc.CAPACITY)
    assert ctx.registry_prove_slots(slots)[2] == [tm.path(lv, s) for s in slots]
    assert old_ids(ctx) == before  # root and prove_slots: none of 27-31
    assert ctx.registry_prove_peers(f)[:3] == (slots, [tm.path(lv, s) for s in slots], [True] * 4)
    assert old_ids(ctx) == before[:3] + (before[3] + 1, before[4])  # the lookup of prove_peers, on the current index
    mid = old_ids(ctx)
    assert neighbours() == first
    assert tuple(b - a for a, b in zip(mid, old_ids(ctx))) == (0, 1, 0, 3, 1)
    assert tree_ids(ctx, api) == (1, 1, 2)
    # a mutation between: the index and the tree are rebuilt independently of each other
    ctx.registry_evict([slots[1]])
    assert ctx.registry_prove_peers(f)[0] == [slots[0], -1, slots[2], slots[3]]
    assert tree_ids(ctx, api) == (2, 2, 3) and old_ids(ctx)[2] == mid[2] + 1
    ctx.registry_admit([rc.pks(k)[97]], [slots[1]])
    assert ctx.registry_root()[0] == tm.root(lv) and neighbours() == first
    ctx.close()
    out = gpu_child("from tests.gpu_child_registry_tree import cohort_member as f; f(2)")
    assert "cohort_member ok 2" in out


def test_registry_audit_example(torch_cuda):
    """9. examples/registry_audit 3 8 prints only lines ending in "= 1" """
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "registry_audit")
    if not os.path.exists(exe):
        pytest.fail("examples/registry_audit missing: run __graft_entry__.build()")
    r = subprocess.run([exe, "3", "8"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 7 and all(ln.endswith("= 1") for ln in lines), r.stdout
    assert lines[-1] == "[result] registry_audit success = 1"
