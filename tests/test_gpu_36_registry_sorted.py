"""GPU tests of the sorted tree (include/kosk_mi355x.h: kosk_registry_sorted_root, kosk_registry_prove_absent, kosk_regsort_order_device;
INTEGRATION.md 8.6, format kosk-regsort-v1) against the hashlib model of tests/registry_sorted_model.py and the host verifier
kosk_regsort_check_proof.  Every comparison is exact."""
import ctypes as C
import hashlib
import itertools
import os
import random
import subprocess

import pytest

from tests import registry_cases as rc
from tests import registry_index_model as rm
from tests import registry_sorted_model as sm
from tests import registry_tree_model as tm

pytestmark = pytest.mark.gpu

KS = rc.KS
SENTINEL = 0xA5
TILE_LG = 11  # REGSORT_TILE_LG of csrc/kosk_ctx.hpp
TILE = 1 << TILE_LG
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
    return api


def key(api, k, tag):
    """any bytes of the right length are a key to kosk_registry_admit"""
    return hashlib.shake_256(b"registry-sorted:%d:" % k + tag).digest(api.pk_bytes(k))


def sort_ids(ctx, api):
    return tuple(ctx.path_count(i) for i in (api.Kosk.PATH_REGSORT_SORT, api.Kosk.PATH_REGSORT_TREE, api.Kosk.PATH_REGSORT_PROVE))


def old_ids(ctx):
    return tuple(ctx.path_count(i) for i in range(27, 35))


def sort_launches(lg, tile_lg=TILE_LG, two=True):
    """k_regsort_keys, the tile launch, and per phase above the tile its steps (two a launch where two are left) and the finishing launch"""
    n = 2
    for p in range(tile_lg + 1, lg + 1):
        n += ((p - tile_lg + 1) // 2 if two else p - tile_lg) + 1
    return n


def queries_of(hs):
    """00^32, FF^32, every key and every key +- 1"""
    out = [ZERO, ONES]
    for h in hs:
        out += [h] + sm.neighbours(h)
    return out


def check_proofs(ctx, api, k, capacity, content, queries):
    """the root, and for each query the kind and the whole record against the model over content = {slot: h}; each record through the host
    verifier, which agrees on the kind; a PRESENT record names the lowest slot that holds the query"""
    d = tm.depth(capacity)
    lv = sm.levels(k, capacity, content)
    want_root = sm.root(lv)
    assert ctx.registry_sorted_root() == (want_root, len(content), capacity)
    kinds, records, root = ctx.registry_prove_absent(queries)
    assert root == want_root and len(records) == len(queries)
    for b, x in enumerate(queries):
        kind, rec = sm.prove(k, capacity, content, x, lv)
        assert kinds[b] == kind and records[b] == rec, (b, x.hex())
        assert api.regsort_check_proof(k, d, x, records[b], root) == kind == sm.check(k, d, x, rec, root), (b, x.hex())
        holders = [s for s, h in content.items() if h == x]
        assert (kind == sm.PRESENT) == bool(holders)
        if holders:
            assert int.from_bytes(rec[4:8], "little") == min(holders)
    return want_root


def small_patterns():
    out = []
    for capacity in (1, 2, 3):
        out += [(capacity, bits) for bits in itertools.product((0, 1), repeat=capacity)]
    out += [(5, bits) for bits in ((0, 0, 0, 0, 0), (1, 1, 1, 1, 1), (1, 0, 0, 0, 1), (0, 1, 1, 0, 0), (0, 0, 0, 0, 1))]
    out += [(8, bits) for bits in ((0,) * 8, (1,) * 8, (1, 0, 1, 0, 1, 0, 1, 0), (0, 0, 0, 1, 1, 0, 0, 0), (0, 0, 0, 0, 0, 0, 0, 1))]
    return out


def test_small_patterns(api):
    """1. capacities 1, 2, 3 with every occupancy pattern, 5 and 8 with a handful, k = 2, one pattern again for k = 3 and 4: the root, and
    proofs for 00^32, FF^32, every key and every key +- 1.  The empty registry (position 0 is Z), the full one (no right record behind
    position P - 1) and D = 0 are among them"""
    roots = {}
    again = [(5, (1, 0, 0, 0, 1))]
    for k, patterns in ((2, small_patterns()), (3, again), (4, again)):
        ctx = api.Kosk(kyber_k=k, max_batch=3)
        for capacity, bits in patterns:
            ctx.registry_reserve(capacity)
            pks = {s: key(api, k, b"small:%d" % s) for s in range(capacity) if bits[s]}
            if pks:
                ctx.registry_admit(list(pks.values()), list(pks))
            content = {s: rm.fp(p) for s, p in pks.items()}
            roots[(k, capacity, bits)] = check_proofs(ctx, api, k, capacity, content, queries_of(content.values()))
            if pks:
                ctx.registry_evict(list(pks))
        ctx.close()
    assert roots[(2, 1, (0,))] == sm.PAD[2] and roots[(2, 2, (0, 0))] == sm.node(sm.PAD[2], sm.PAD[2])
    assert len({roots[(k, 5, (1, 0, 0, 0, 1))] for k in KS}) == 3


@pytest.mark.parametrize("capacity,full", ((TILE, False), (TILE + 1, False), (4 * TILE, False), (TILE, True)))
def test_tile_edges(capacity, full, api):
    """2. one tile; one tile and one slot (two tiles, one global step); four tiles (the two-step launch); about a third of the slots
    occupied, and one tile fully occupied (no padding, no right record behind the last key).  The root against the model; proofs at the
    first, the last and the tile-boundary positions, with their neighbours"""
    k = 2
    occupied = list(range(capacity)) if full else sorted({(s * 7919 + 3) % capacity for s in range(capacity // 3)} | {0, capacity - 1})
    pks = [key(api, k, b"tile:%d" % s) for s in occupied]
    content = {s: rm.fp(p) for s, p in zip(occupied, pks)}
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(capacity)
    ctx.registry_admit(pks, occupied)
    ent = sm.entries(content)
    at = sorted({0, 1, len(ent) - 1} | {p for p in (TILE - 1, TILE, 2 * TILE - 1, 2 * TILE) if p < len(ent)})
    before = sort_ids(ctx, api)
    check_proofs(ctx, api, k, capacity, content, queries_of([ent[p][0] for p in at]))
    d = tm.depth(capacity)
    assert sort_ids(ctx, api) == (before[0] + sort_launches(d), before[1] + max(1, -(-d // 10)), before[2] + 1)
    ctx.close()


def test_duplicates(api):
    """3. one key in slots 6, 1 and 4 of 8 through kosk_registry_admit: three adjacent entries in slot order; PRESENT names slot 1, after
    its eviction slot 4"""
    k = 2
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(8)
    pk, low, high = key(api, k, b"dup"), key(api, k, b"dup:a"), key(api, k, b"dup:b")
    h = rm.fp(pk)
    pks = {6: pk, 1: pk, 4: pk, 0: low, 7: high}
    ctx.registry_admit(list(pks.values()), list(pks))
    content = {s: rm.fp(p) for s, p in pks.items()}
    ent = sm.entries(content)
    first = ent.index((h, 1))
    assert ent[first:first + 3] == [(h, 1), (h, 4), (h, 6)]
    root = check_proofs(ctx, api, k, 8, content, queries_of(content.values()))
    kinds, records, _ = ctx.registry_prove_absent([h])
    assert kinds == [sm.PRESENT] and int.from_bytes(records[0][:4], "little") == first and int.from_bytes(records[0][4:8], "little") == 1
    assert ctx.registry_find([h]) == [1]
    # the neighbours of the run: the key below it ends at the run's first entry, the key above it starts behind its last
    below, above = sm.neighbours(h)
    recs = ctx.registry_prove_absent([below, above])[1]
    assert int.from_bytes(recs[0][8:12], "little") == 1 and int.from_bytes(recs[1][4:8], "little") == 6
    ctx.registry_evict([1])
    del content[1]
    assert check_proofs(ctx, api, k, 8, content, queries_of(content.values())) != root
    assert int.from_bytes(ctx.registry_prove_absent([h])[1][0][4:8], "little") == 4
    ctx.close()


def crafted(n, rng):
    """name -> n fingerprints"""
    base = rng.randbytes(32)
    out = {"equal": [base] * n, "ascending": [(i * 2 ** 200 + 5).to_bytes(32, "big") for i in range(n)],
           "random": [rng.randbytes(32) for _ in range(n)]}
    out["descending"] = out["ascending"][::-1]
    out["random"][0] = ZERO
    out["random"][-1] = ONES
    if n > 2:
        out["random"][n // 2] = ZERO  # 00^32 twice, in the order of the indices
    for agree in (8, 16, 24, 31):
        out["agree%d" % agree] = [base[:agree] + rng.randbytes(32 - agree) for _ in range(n)]
    # the differing byte right behind the prefix, descending, so every comparison of two records is decided by the bytes the records lack
    out["tail"] = [base[:8] + ((n - 1 - i) * 2 ** 100).to_bytes(24, "big") for i in range(n)]
    return out


@pytest.mark.parametrize("n", (1, 2, 3, TILE - 1, TILE, TILE + 1, 3 * TILE + 5))
def test_crafted_fingerprints(n, api, torch_cuda, monkeypatch):
    """4. kosk_regsort_order_device against Python's sorted: fingerprints no SHA3 would give -- all equal, agreeing in the first 8, 16, 24
    and 31 bytes, ascending, descending, random with 00^32 and FF^32 among them -- under flags all 1, all 0 and mixed; at the largest n also
    with every step above the tile in a launch of its own, and with the tiles of 2^10 and 2^12 records that the measurement compares"""
    torch = torch_cuda
    rng = random.Random(3600 + n)
    ctx = api.Kosk(kyber_k=2, max_batch=1)
    d_order = torch.empty((n,), dtype=torch.int32, device="cuda")
    lg = (n - 1).bit_length()
    settings = ((11, 1), (11, 0), (10, 1), (12, 1)) if n > 2 * TILE else ((11, 1),)
    for tile_lg, step2 in settings:
        monkeypatch.setenv("KOSK_DEBUG_REGSORT_TILE_LG", str(tile_lg))
        monkeypatch.setenv("KOSK_DEBUG_REGSORT_STEP2", str(step2))
        for name, hs in crafted(n, rng).items():
            d_h = torch.frombuffer(bytearray(b"".join(hs)), dtype=torch.uint8).cuda()
            for flags in ([1] * n, [0] * n, [rng.randrange(2) for _ in range(n)]):
                d_flag = torch.tensor(flags, dtype=torch.uint8, device="cuda")
                d_order.fill_(-7)
                torch.cuda.synchronize()
                before = sort_ids(ctx, api)
                ctx.regsort_order(n, d_h.data_ptr(), d_flag.data_ptr(), d_order.data_ptr())
                want = [i for _, i in sorted((hs[i], i) for i in range(n) if flags[i])]
                assert d_order.cpu().tolist() == want + [-1] * (n - len(want)), (name, tile_lg, step2, sum(flags))
                assert sort_ids(ctx, api) == (before[0] + sort_launches(lg, tile_lg, bool(step2)), before[1], before[2])
                assert bytes(d_h.cpu().numpy()) == b"".join(hs)
    ctx.close()


def test_invalidation(api):
    """5. admit, evict, enrol and a new reserve each cause exactly one rebuild (ids 35 and 36), a second call on a current tree none; ids
    27..34, the slot tree's root and kosk_kem_enc_peers are what they were"""
    k, capacity = 2, 2 * TILE
    d = tm.depth(capacity)
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(capacity)
    pks = {s: rc.pks(k)[i] for i, s in enumerate((0, 5, 2047, 2048, 4095))}
    ctx.registry_admit(list(pks.values()), list(pks))
    coins = list(rc.messages(k)[:2])
    peers = [rm.fp(pks[5]), rm.fp(pks[2048])]

    def content():
        return {s: rm.fp(p) for s, p in pks.items()}

    def step(rebuilds, cap=capacity):
        slot_root, enc = ctx.registry_root(), ctx.kem_enc_peers(peers, coins)
        before, old = sort_ids(ctx, api), old_ids(ctx)
        root, used, c_ = ctx.registry_sorted_root()
        kinds, records, root2 = ctx.registry_prove_absent([ZERO, peers[0]])
        dd = tm.depth(cap)
        assert sort_ids(ctx, api) == (before[0] + rebuilds * sort_launches(dd), before[1] + rebuilds * max(1, -(-dd // 10)), before[2] + 1)
        assert old_ids(ctx) == old
        assert (root, used, c_) == (sm.root(sm.levels(k, cap, content())), len(pks), cap) and root2 == root
        assert kinds == [sm.ABSENT, sm.PRESENT] and int.from_bytes(records[1][4:8], "little") == min(s for s, p in pks.items() if rm.fp(p) == peers[0])
        assert ctx.registry_root() == slot_root and ctx.kem_enc_peers(peers, coins) == enc
        return root
    roots = [step(1), step(0)]
    assert roots[0] == roots[1]
    pks[77] = rc.pks(k)[9]
    ctx.registry_admit([pks[77]], [77])
    roots.append(step(1))
    roots.append(step(0))
    ctx.registry_evict([0])
    del pks[0]
    roots.append(step(1))
    new = [key(api, k, b"inv:%d" % i) for i in range(2)]
    slots, status = ctx.registry_enrol(new)
    assert slots == [0, 1] and status == [rm.ADMITTED] * 2
    pks.update(dict(zip(slots, new)))
    roots.append(step(1))
    assert len(set(roots)) == 4
    ctx.registry_evict(list(pks))
    moved = sort_ids(ctx, api)
    ctx.registry_reserve(5)
    assert sort_ids(ctx, api) == moved  # reserve itself builds nothing
    pks.clear()
    pks[3] = rc.pks(k)[9]
    pks[1] = rc.pks(k)[5]
    ctx.registry_admit(list(pks.values()), list(pks))
    peers[:] = [rm.fp(pks[3]), rm.fp(pks[1])]
    step(1, cap=5)
    step(0, cap=5)
    ctx.close()


def test_buffers_across_a_launch_group(api, torch_cuda):
    """6. 16 385 queries at capacity 5: host buffers, and device buffers at odd byte offsets between sentinel bytes; id 37 moves by two"""
    torch = torch_cuda
    k, capacity, n = 3, 5, rc.CHUNK + 1
    d = tm.depth(capacity)
    rec = sm.proof_bytes(d)
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(capacity)
    pks = {4: key(api, k, b"buf:4"), 0: key(api, k, b"buf:0"), 2: key(api, k, b"buf:2")}
    ctx.registry_admit(list(pks.values()), list(pks))
    content = {s: rm.fp(p) for s, p in pks.items()}
    lv = sm.levels(k, capacity, content)
    distinct = queries_of(content.values()) + [hashlib.sha3_256(b"buf-absent:%d" % i).digest() for i in range(30)]
    answers = {x: sm.prove(k, capacity, content, x, lv) for x in distinct}
    hs = [distinct[(b * 7 + b // 41) % len(distinct)] for b in range(n)]
    want_kinds = [answers[x][0] for x in hs]
    want_records = b"".join(answers[x][1] for x in hs)
    ctx.registry_sorted_root()
    before = sort_ids(ctx, api)
    kinds, records, root = ctx.registry_prove_absent(hs)
    assert sort_ids(ctx, api) == (before[0], before[1], before[2] + 2)
    assert kinds == want_kinds and b"".join(records) == want_records and root == sm.root(lv)
    for b in sorted({0, 1, rc.CHUNK - 1, rc.CHUNK, n - 1} | set(range(0, n, 499))):
        assert api.regsort_check_proof(k, d, hs[b], records[b], root) == want_kinds[b], b
    sizes = (n, rec * n, 32)
    offs = (3, 1, 5)
    d_h = torch.frombuffer(bytearray(b"\x00" + b"".join(hs)), dtype=torch.uint8).cuda()
    outs = [torch.full((off + size + 8,), SENTINEL, dtype=torch.uint8, device="cuda") for off, size in zip(offs, sizes)]
    torch.cuda.synchronize()
    ctx.registry_prove_absent(d_h.data_ptr() + 1, n=n, out=tuple(t.data_ptr() + off for t, off in zip(outs, offs)))
    for t, off, want in zip(outs, offs, (bytes(want_kinds), want_records, root)):
        assert bytes(t.cpu().numpy()) == bytes([SENTINEL]) * off + want + bytes([SENTINEL]) * 8
    assert bytes(d_h.cpu().numpy()) == b"\x00" + b"".join(hs)
    # the root to device memory, and no root at all
    d_root = torch.full((1 + 32 + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.registry_sorted_root(out=d_root.data_ptr() + 1)[1:] == (3, 5)
    assert bytes(d_root.cpu().numpy()) == bytes([SENTINEL]) + root + bytes([SENTINEL]) * 8
    kind, one = C.create_string_buffer(1), C.create_string_buffer(rec)
    assert api.lib.kosk_registry_prove_absent(ctx.handle, 1, C.c_char_p(hs[0]), kind, one, None) == 0
    assert (kind.raw[0], one.raw) == answers[hs[0]]
    ctx.close()


def test_refusals(api, torch_cuda):
    """7. NULL arguments, n < 1, no registry, n above 2^24 and a misaligned pointer for the order: -1, a text that begins with the call's
    name, counters unchanged; the handle still works"""
    torch = torch_cuda
    k = 3
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    lib, h = api.lib, ctx.handle
    pk = rc.pks(k)[0]
    fp = rm.fp(pk)

    def snapshot():
        return rc.counts(ctx, api) + old_ids(ctx) + sort_ids(ctx, api)
    for name, fn in (("registry_sorted_root", lambda: ctx.registry_sorted_root()), ("registry_prove_absent", lambda: ctx.registry_prove_absent([fp]))):
        before = snapshot()
        with pytest.raises(api.KoskError, match="kosk_%s: .*no registry is reserved" % name):
            fn()
        assert snapshot() == before
    ctx.registry_reserve(4)
    ctx.registry_admit([pk], [1])
    before = snapshot()
    buf = C.create_string_buffer(512)
    for n in (0, -1):
        assert lib.kosk_registry_prove_absent(h, n, buf, buf, buf, buf) == -1
    assert lib.kosk_registry_sorted_root(h, None, None, None) == -1 and b"kosk_registry_sorted_root: invalid argument" in lib.kosk_last_error(h)
    assert lib.kosk_registry_prove_absent(h, 1, None, buf, buf, buf) == -1 and b"kosk_registry_prove_absent: invalid argument" in lib.kosk_last_error(h)
    assert lib.kosk_registry_prove_absent(h, 1, buf, None, buf, buf) == -1 and lib.kosk_registry_prove_absent(h, 1, buf, buf, None, buf) == -1
    assert lib.kosk_registry_sorted_root(None, buf, None, None) == -1 and lib.kosk_registry_prove_absent(None, 1, buf, buf, buf, buf) == -1
    dev = torch.zeros((256,), dtype=torch.uint8, device="cuda")
    p = dev.data_ptr()
    order = lib.kosk_regsort_order_device
    assert order(None, 1, p, p + 64, p + 128) == -1
    assert order(h, 0, p, p + 64, p + 128) == -1 and b"kosk_regsort_order_device: invalid argument" in lib.kosk_last_error(h)
    assert order(h, 2 ** 24 + 1, p, p + 64, p + 128) == -1
    assert order(h, 1, None, p + 64, p + 128) == -1 and order(h, 1, p, None, p + 128) == -1 and order(h, 1, p, p + 64, None) == -1
    assert order(h, 1, p + 4, p + 64, p + 128) == -1 and order(h, 1, p, p + 64, p + 130) == -1
    assert snapshot() == before and sort_ids(ctx, api) == (0, 0, 0)
    assert order(h, 2, p, p + 65, p + 128) == 0 and dev[128:136].cpu().tolist() == [255] * 8  # flags 0: two times -1
    assert ctx.registry_prove_absent([fp])[0] == [sm.PRESENT]
    ctx.close()


def test_inventory_and_erasure(api):
    """8. the sorted records, the tree and the staging are public buffers of the inventory from the first call on; the wipes leave them
    alone; the staged queries are gone when the call returns; after an eviction and the next call nothing of the evicted key is left"""
    k = 2
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(5)
    pk_a, pk_b = rc.pks(k)[3], rc.pks(k)[4]
    fa, fb = rm.fp(pk_a), rm.fp(pk_b)
    ctx.registry_admit([pk_a, pk_b], [1, 3])
    content = {1: fa, 3: fb}
    assert ctx.secret_scan(sm.PAD[k]) == 0 and ctx.secret_scan(sm.leaf(k, fa, 1)) == 0
    lv = sm.levels(k, 5, content)
    root = ctx.registry_sorted_root()[0]
    assert root == sm.root(lv)
    assert ctx.secret_scan(sm.PAD[k]) == 6  # positions 2..7, before any record is staged
    assert ctx.secret_scan(sm.leaf(k, fa, 1)) == 1 and ctx.secret_scan(root) == 1 and ctx.secret_scan(fa) == 1
    sort_record = fa[:8][::-1] + (1).to_bytes(4, "little") + bytes(4)  # the prefix as a number, the slot, class 0
    assert ctx.secret_scan(sort_record) == 1
    nobody = hashlib.sha3_256(b"sorted-nobody").digest()
    proved = ctx.registry_prove_absent([fa, nobody, ZERO])
    assert proved[0] == [sm.PRESENT, sm.ABSENT, sm.ABSENT]
    assert ctx.secret_scan(nobody) == 0  # the staged queries are gone
    assert ctx.secret_scan(fa) >= 2  # the slot, and the records that carry it
    built = sort_ids(ctx, api)
    ctx.wipe_secrets()
    assert ctx.registry_sorted_root()[0] == root and ctx.registry_prove_absent([fa, nobody, ZERO]) == proved
    ctx.set_wipe(api.WIPE_CALL)
    assert ctx.kem_enc_slots([1, 3], list(rc.messages(k)[3:5]))[2] == [True, True]
    assert ctx.registry_sorted_root()[0] == root and ctx.registry_prove_absent([fa, nobody, ZERO]) == proved
    ctx.set_wipe(api.WIPE_OFF)
    assert sort_ids(ctx, api)[:2] == built[:2]  # nothing was rebuilt
    ctx.registry_evict([1])
    lv2 = sm.levels(k, 5, {3: fb})
    assert ctx.registry_sorted_root() == (sm.root(lv2), 1, 5)
    # gone from the slot, the sorted records, the tree and the records staged from the earlier state
    assert ctx.secret_scan(sm.leaf(k, fa, 1)) == 0 and ctx.secret_scan(fa) == 0 and ctx.secret_scan(sort_record) == 0
    assert ctx.secret_scan(sm.leaf(k, fb, 3)) == 1
    kinds, records, root2 = ctx.registry_prove_absent([fa])
    assert kinds == [sm.ABSENT] and api.regsort_check_proof(k, 3, fa, records[0], root2) == sm.ABSENT
    # reserve drops the sorted tree with the registry
    ctx.registry_evict([3])
    ctx.registry_reserve(2)
    assert ctx.secret_scan(sm.PAD[k]) == 0
    assert ctx.registry_sorted_root() == (sm.node(sm.PAD[k], sm.PAD[k]), 0, 2) and ctx.secret_scan(sm.PAD[k]) == 2
    ctx.close()


def test_cohort_member_in_a_child_process(gpu_child):
    """9. a cohort member, unmerged, in a fresh child process"""
    out = gpu_child("from tests.gpu_child_registry_sorted import cohort_member as f; f(2)")
    assert "cohort_member ok 2" in out


def test_registry_absent_example(torch_cuda):
    """10. examples/registry_absent 3 8 prints only lines ending in "= 1" """
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "registry_absent")
    if not os.path.exists(exe):
        pytest.fail("examples/registry_absent missing: run __graft_entry__.build()")
    r = subprocess.run([exe, "3", "8"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 6 and all(ln.endswith("= 1") for ln in lines), r.stdout
    assert lines[-1] == "[result] registry_absent success = 1"
