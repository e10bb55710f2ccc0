"""GPU tests of the registry by fingerprint (include/kosk_mi355x.h: kosk_registry_find, kosk_registry_enrol, kosk_registry_enrol_verified,
kosk_kem_enc_peers) against the model of tests/registry_index_model.py, against tests/golden/kem_vectors_v1.json --
what the reference's crypto_kem_enc_derand returned for 130 distinct keys --, against kosk_kem_enc_slots on the same handle, which
tests/test_gpu_32_registry.py pins to that fixture, and against hashlib for the fingerprints.  Every comparison is exact."""
import ctypes as C
import hashlib
import os
import subprocess

import pytest

from tests import kem_fixture as kf
from tests import registry_cases as rc
from tests import registry_index_model as rm

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
    """one handle per K with the fixture's 130 keys admitted, key i in slot(i); the tests that change the registry make their own"""
    hs = {k: api.Kosk(kyber_k=k, max_batch=3) for k in KS}
    for k, h in hs.items():
        rc.admit_fixture(h, k)
    yield hs
    for h in hs.values():
        h.close()


def fps(k):
    """the fingerprints of the 130 fixture keys, from hashlib"""
    return [rm.fp(p) for p in rc.pks(k)]


def absent(tag):
    """a fingerprint no fixture key has"""
    return hashlib.sha3_256(b"registry-index-absent:%d" % tag).digest()


def ids(ctx, api):
    return tuple(ctx.path_count(i) for i in (api.Kosk.PATH_REGISTRY_INDEX, api.Kosk.PATH_REGISTRY_FIND, api.Kosk.PATH_KEM_ENC_PEERS))


@pytest.mark.parametrize("capacity", (1, 2, 3, 8))
def test_probe_chains_and_wrap_around(capacity, api):
    """1. T = 2, 4, 8, 16: keys ground so that all share one home; so that the home is entry T - 1 and the chain wraps; so that two clusters
    abut.  find of every admitted fingerprint, and of absent fingerprints ground onto the same homes: their walk crosses a full cluster to
    the empty entry.  Keys enter highest slot first, so a chain's order is not the slots' order"""
    k = 2
    size = api.pk_bytes(k)
    t = rm.entries(capacity)
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(capacity)
    a = capacity // 2
    layouts = [[(t // 2, capacity)], [(t - 1, capacity)]]
    if a:
        layouts.append([(t - 1, a), ((t - 1 + a) % t, capacity - a)])  # cluster 1 wraps and fills entries T-1 .. ; cluster 2's home is the entry behind it
    for layout in layouts:
        model = rm.Model(capacity)
        keys, ghosts = [], []
        for home, count in layout:
            keys += rm.grind(capacity, home, count, size)
            ghosts += rm.grind(capacity, home, 2, size, tag=b"absent")
        assert len(set(keys)) == capacity and not set(keys) & set(ghosts)
        slots = list(range(capacity))[::-1]
        ctx.registry_admit(keys, slots)
        model.admit(keys, slots)
        assert ctx.registry_find([rm.fp(p) for p in keys]) == slots == [model.find(rm.fp(p)) for p in keys]
        assert ctx.registry_find([rm.fp(p) for p in ghosts]) == [-1] * len(ghosts)
        mixed = [rm.fp(p) for pair in zip(ghosts, keys * 2) for p in pair]
        assert ctx.registry_find(mixed) == [model.find(h) for h in mixed]
        # one key leaves the middle of the chain: the rest are still found behind the hole of the rebuilt table
        gone = slots[len(slots) // 2]
        ctx.registry_evict([gone])
        model.evict([gone])
        assert ctx.registry_find([rm.fp(p) for p in keys]) == [model.find(rm.fp(p)) for p in keys]
        ctx.registry_evict(slots)
        assert ctx.registry_find([rm.fp(p) for p in keys]) == [-1] * capacity
    ctx.close()


def test_duplicates_through_the_existing_call(api):
    """2. one key admitted with kosk_registry_admit to slots 5, 2 and 7 of 8: find gives 2; evict 2: 5; evict all: -1; re-admit: found
    again.  Every lookup after a mutation rebuilds (id 29), a lookup without one does not"""
    k = 2
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(8)
    pk, other = rc.pks(k)[7], rc.pks(k)[8]
    h = rm.fp(pk)
    rebuilds = api.Kosk.PATH_REGISTRY_INDEX
    ctx.registry_admit([pk, pk, pk, other], [5, 2, 7, 0])
    assert ctx.registry_find([h, rm.fp(other)]) == [2, 0] and ctx.path_count(rebuilds) == 1
    assert ctx.registry_find([h]) == [2] and ctx.path_count(rebuilds) == 1
    ctx.registry_evict([2])
    assert ctx.registry_find([h]) == [5] and ctx.path_count(rebuilds) == 2
    ctx.registry_evict([5, 7])
    assert ctx.registry_find([h, rm.fp(other)]) == [-1, 0] and ctx.path_count(rebuilds) == 3
    ctx.registry_evict([0])
    assert ctx.registry_find([h, rm.fp(other)]) == [-1, -1] and ctx.path_count(rebuilds) == 4
    ctx.registry_admit([pk], [6])
    assert ctx.registry_find([h]) == [6] and ctx.path_count(rebuilds) == 5
    ctx.registry_admit([pk], [3])
    assert ctx.registry_find([h]) == [3] and ctx.path_count(rebuilds) == 6
    ctx.registry_evict([3, 6])
    ctx.registry_reserve(4)  # a new registry: a new index
    ctx.registry_admit([pk], [3])
    assert ctx.registry_find([h]) == [3] and ctx.path_count(rebuilds) == 7
    ctx.close()


@pytest.mark.parametrize("n", (1, 63, 64, 65, 130))
@pytest.mark.parametrize("k", KS)
def test_wave_edges(k, n, handles, torch_cuda):
    """3. n queries on the 130 fixture keys at rc.slot(i), every third a miss; host buffers, and device buffers at an odd byte offset"""
    torch = torch_cuda
    ctx = handles[k]
    hs = [absent(b) if b % 3 == 1 else fps(k)[b] for b in range(n)]
    want = [-1 if b % 3 == 1 else rc.slot(b) for b in range(n)]
    assert ctx.registry_find(hs) == want
    d_h = torch.frombuffer(bytearray(b"\x00" + b"".join(hs)), dtype=torch.uint8).cuda()
    d_out = torch.full((3 + 4 * n + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.registry_find(d_h.data_ptr() + 1, n=n, out=d_out.data_ptr() + 3)
    raw = bytes(d_out.cpu().numpy())
    assert raw[:3] == bytes([SENTINEL]) * 3 and raw[3 + 4 * n:] == bytes([SENTINEL]) * 8
    assert [int.from_bytes(raw[3 + 4 * b:7 + 4 * b], "little", signed=True) for b in range(n)] == want
    assert bytes(d_h.cpu().numpy()) == b"\x00" + b"".join(hs)


@pytest.mark.parametrize("k", KS)
def test_enc_peers_equals_the_reference(k, handles):
    """4. the 130 fixture keys by fingerprint: every ct digest and ss equals the fixture's, and the bytes of kosk_kem_enc_slots on
    kosk_registry_find's slots; with misses among them: zeros and done 0"""
    ctx = handles[k]
    coins = list(rc.messages(k))
    cts, sss, done = ctx.kem_enc_peers(fps(k), coins)
    want = rc.items(k)
    assert done == [True] * kf.ITEMS
    for i in range(kf.ITEMS):
        assert kf.sha3(cts[i]) == want[i]["ct"], ("ct", k, i)
        assert sss[i].hex() == want[i]["ss"], ("ss", k, i)
    slots = ctx.registry_find(fps(k))
    assert slots == [rc.slot(i) for i in range(kf.ITEMS)]
    assert (cts, sss, done) == ctx.kem_enc_slots(slots, coins)
    miss = (0, 64, 129)
    hs = [absent(i) if i in miss else fps(k)[i] for i in range(kf.ITEMS)]
    cts2, sss2, done2 = ctx.kem_enc_peers(hs, coins)
    assert done2 == [i not in miss for i in range(kf.ITEMS)]
    for i in range(kf.ITEMS):
        assert (cts2[i], sss2[i]) == ((bytes(kf.CT_BYTES[k]), bytes(32)) if i in miss else (cts[i], sss[i])), i


@pytest.mark.parametrize("k", KS)
def test_coins_from_the_randombytes_callback(k, handles, api):
    """4. coins=None with two misses among 7: exactly 7 draws of 32 bytes, in item order; the results equal the explicit call on what the
    callback returned; a refused call draws none"""
    ctx = handles[k]
    f = fps(k)
    hs = [f[0], f[1], absent(1), f[97], f[24], absent(2), f[0]]
    calls = []

    def rb(nbytes):
        out = hashlib.shake_256(b"registry-index-callback:%d:%d" % (k, len(calls))).digest(nbytes)
        calls.append(out)
        return out
    ctx.set_randombytes(rb)
    try:
        got = ctx.kem_enc_peers(hs)
    finally:
        ctx.set_randombytes(None)
    assert [len(c) for c in calls] == [32] * 7
    assert got == ctx.kem_enc_peers(hs, calls) and len(calls) == 7
    assert got[2] == [True, True, False, True, True, False, True] and got[0][2] == bytes(kf.CT_BYTES[k]) and got[1][5] == bytes(32)
    keys = [0, 1, 97, 24, 0]
    want = ctx.kem_enc([rc.pks(k)[i] for i in keys], calls[:2] + calls[3:5] + calls[6:])
    assert (got[0][:2] + got[0][3:5] + got[0][6:], got[1][:2] + got[1][3:5] + got[1][6:]) == want
    bare = api.Kosk(kyber_k=k, max_batch=3)  # no registry: refused before any coin is drawn
    drawn = []
    bare.set_randombytes(lambda nbytes: drawn.append(nbytes) or bytes(nbytes))
    try:
        with pytest.raises(api.KoskError, match="kosk_kem_enc_peers: .*no registry is reserved"):
            bare.kem_enc_peers(hs)
    finally:
        bare.set_randombytes(None)
    assert drawn == [] and ids(bare, api) == (0, 0, 0)
    bare.close()


@pytest.mark.parametrize("n", (rc.CHUNK, rc.CHUNK + 1))
def test_launch_groups(n, handles, api):
    """5. kosk_kem_enc_peers and kosk_registry_find of 16 384 and 16 385 items on the 130-key registry, fingerprints modulo 130 with every
    97th a miss: the first and last item of each group and a sample; ids 30 and 31 move by 1 and by 2"""
    k = 3
    ctx = handles[k]
    groups = 1 if n <= rc.CHUNK else 2
    idx = [b % kf.ITEMS for b in range(n)]
    f, msgs = fps(k), rc.messages(k)
    hs = [absent(b) if b % 97 == 96 else f[idx[b]] for b in range(n)]
    assert ctx.registry_find(f[:1]) == [rc.slot(0)]  # the index is current from here on
    before = ids(ctx, api)
    slots = ctx.registry_find(hs)
    after = ids(ctx, api)
    assert after == (before[0], before[1] + groups, before[2])
    assert slots == [-1 if b % 97 == 96 else rc.slot(idx[b]) for b in range(n)]
    cts, sss, done = ctx.kem_enc_peers(hs, [msgs[i] for i in idx])
    assert ids(ctx, api) == (after[0], after[1] + groups, after[2] + groups)
    assert done == [b % 97 != 96 for b in range(n)]
    want = rc.items(k)
    probe = sorted({0, 1, 95, 96, 97, rc.CHUNK - 2, rc.CHUNK - 1, n - 1} | set(range(0, n, 1009)))
    assert any(b % 97 == 96 for b in probe)
    for b in probe:
        if b % 97 == 96:
            assert cts[b] == bytes(kf.CT_BYTES[k]) and sss[b] == bytes(32), b
        else:
            assert kf.sha3(cts[b]) == want[idx[b]]["ct"] and sss[b].hex() == want[idx[b]]["ss"], b


def test_enrol_against_the_model(api):
    """6. capacity 8 with slots 1 and 4 occupied: mixed accept bytes, duplicates within the call, a rejected first occurrence, duplicates of
    keys already present; slots are given out in ascending order around the occupied ones; the full-registry refusal changes nothing"""
    k = 2
    p = rc.pks(k)
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    model = rm.Model(8)
    ctx.registry_reserve(8)
    ctx.registry_admit([p[10], p[11]], [4, 1])
    model.admit([p[10], p[11]], [4, 1])
    cand = [p[20], p[20], p[11], p[21], p[20], p[22], p[10], p[21], p[23]]
    accept = [0, 1, 1, 1, 1, 0, 1, 1, 1]
    want = model.enrol(cand, accept)
    assert want == ([-1, 0, 1, 2, 0, -1, 4, 2, 3], [0, 1, 2, 1, 2, 0, 2, 2, 1])
    assert ctx.registry_enrol(cand, accept) == want and ctx.registry_level() == (5, 8)
    states, got_pk, got_h = ctx.registry_read(list(range(8)))
    assert states == [1, 1, 1, 1, 1, 0, 0, 0] and got_pk[:5] == [p[20], p[11], p[21], p[23], p[10]] == model.slots[:5]
    assert got_h[:5] == [rm.fp(x) for x in model.slots[:5]]
    assert ctx.registry_find([rm.fp(x) for x in cand]) == [model.find(rm.fp(x)) for x in cand] == [0, 0, 1, 2, 0, -1, 4, 2, 3]
    # four new keys (one of them twice), three empty slots
    full = [p[30], p[31], p[30], p[32], p[20], p[33]]
    before = (ctx.registry_read(list(range(8))), ctx.registry_level(), ctx.path_count(api.Kosk.PATH_REGISTRY_ADMIT))
    assert model.enrol(full) is None
    with pytest.raises(api.KoskError, match="kosk_registry_enrol: .*registry is full"):
        ctx.registry_enrol(full)
    assert (ctx.registry_read(list(range(8))), ctx.registry_level(), ctx.path_count(api.Kosk.PATH_REGISTRY_ADMIT)) == before
    # accept = None, exactly as many new keys as empty slots; the admitted keys serve encapsulations
    want = model.enrol(full[:5])
    assert want == ([5, 6, 5, 7, 0], [1, 1, 2, 1, 2])
    assert ctx.registry_enrol(full[:5]) == want and ctx.registry_level() == (8, 8)
    coins = list(rc.messages(k)[:3])
    assert ctx.kem_enc_peers([rm.fp(p[32]), rm.fp(p[20]), rm.fp(p[33])], coins)[2] == [True, True, False]
    assert ctx.kem_enc_peers([rm.fp(p[32]), rm.fp(p[20])], coins[:2])[:2] == ctx.kem_enc([p[32], p[20]], coins[:2])
    # only duplicates and rejections: nothing is admitted, no launch of k_registry_admit
    admits = ctx.path_count(api.Kosk.PATH_REGISTRY_ADMIT)
    assert ctx.registry_enrol([p[30], p[99]], [1, 0]) == ([5, -1], [2, 0]) and ctx.path_count(api.Kosk.PATH_REGISTRY_ADMIT) == admits
    ctx.close()


def _verified_handle(api, oracle, k, first_tape):
    """a handle whose last verify call covered three proofs, proof 1 tampered: bits [1, 0, 1]"""
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    pks, sks, pis = ctx.verifiable_keygen([oracle.tape_bytes_for(k, first_tape + i) for i in range(3)])
    bad = bytearray(pis[1]); bad[1000] ^= 1
    pis = [pis[0], bytes(bad), pis[2]]
    assert ctx.verify(pis, pks) == [True, False, True]
    return ctx, pks, sks, pis


def test_enrol_verified(api, oracle):
    """7. the keys of a verify call with bits [1, 0, 1]: slots [0, -1, 1], the tampered one REJECTED; once more after the same verify
    call: DUPLICATE in the same slots; encapsulation by fingerprint equals kosk_kem_enc_verified where the bit is 1"""
    k = 2
    coins = [hashlib.shake_256(b"registry-index-verified:%d" % i).digest(32) for i in range(3)]
    ctx, pks, sks, pis = _verified_handle(api, oracle, k, 40)
    ctx.registry_reserve(8)
    assert ctx.registry_enrol_verified(3) == ([0, -1, 1], [rm.ADMITTED, rm.REJECTED, rm.ADMITTED])
    assert ctx.registry_level() == (2, 8)
    assert ctx.registry_read([0, 1, 2])[:2] == ([1, 1, 0], [pks[0], pks[2], bytes(ctx.pk_bytes)])
    assert ctx.registry_enrol_verified(3) == ([0, -1, 1], [rm.DUPLICATE, rm.REJECTED, rm.DUPLICATE]) and ctx.registry_level() == (2, 8)
    assert ctx.registry_enrol_verified(1) == ([0], [rm.DUPLICATE])
    got = ctx.kem_enc_peers([rm.fp(p) for p in pks], coins)
    assert got == ctx.kem_enc_verified(3, coins) and got[2] == [True, False, True]
    assert ctx.kem_dec([got[0][0], got[0][2]], [sks[0], sks[2]]) == [got[1][0], got[1][2]]
    ctx.close()


def test_enrol_verified_refusals(api, oracle):
    """7. every refusal of kosk_registry_admit_verified under the new name: -1, the call's name, level and counters unchanged"""
    k = 2
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    tapes = [oracle.tape_bytes_for(k, 40 + i) for i in range(3)]

    def refused(text):
        before = rc.counts(ctx, api) + ids(ctx, api)
        with pytest.raises(api.KoskError, match="kosk_registry_enrol_verified: .*" + text):
            ctx.registry_enrol_verified(3)
        assert rc.counts(ctx, api) + ids(ctx, api) == before
    refused("no registry is reserved")
    ctx.registry_reserve(8)
    refused("no verify call")
    pks, sks, pis = ctx.verifiable_keygen(tapes)
    refused("no verify call")
    ctx.stage_verifier_inputs(pis[:2], pks[:2])
    assert ctx.verify_resident(2) == [True, True]
    refused("fewer than n")
    assert ctx.verify(pis + pis[:1], pks + pks[:1]) == [True] * 4
    refused("chunked")
    assert ctx.verify(pis, pks) == [True] * 3
    ctx.stage_verifier_inputs(pis, pks)
    refused("replaced")
    assert ctx.verify(pis, pks) == [True] * 3
    ctx.verifiable_keygen(tapes[:1])
    refused("replaced")
    ctx.verifiable_keygen(tapes)
    assert ctx.verify_inst(pis, [rc.inst(api, k, t[:64]) for t in tapes]) == [True] * 3
    refused("no public key bytes")
    assert ctx.verify(pis, pks) == [True] * 3
    assert ctx.registry_enrol_verified(3) == ([0, 1, 2], [rm.ADMITTED] * 3) and ctx.registry_level() == (3, 8)  # the handle still works
    ctx.close()


def test_refusals(api):
    """NULL arguments, n < 1 and no registry: -1, a text that begins with the call's name, nothing started"""
    k = 3
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    lib, h = api.lib, ctx.handle
    pk, fp = rc.pks(k)[0], rm.fp(rc.pks(k)[0])

    def refused(name, text, fn):
        before = rc.counts(ctx, api) + ids(ctx, api)
        with pytest.raises(api.KoskError, match="kosk_%s: .*%s" % (name, text)):
            fn()
        assert rc.counts(ctx, api) + ids(ctx, api) == before
    refused("registry_find", "no registry is reserved", lambda: ctx.registry_find([fp]))
    refused("registry_enrol", "no registry is reserved", lambda: ctx.registry_enrol([pk]))
    refused("kem_enc_peers", "no registry is reserved", lambda: ctx.kem_enc_peers([fp], [rc.messages(k)[0]]))
    ctx.registry_reserve(4)
    before = rc.counts(ctx, api) + ids(ctx, api)
    slots = (C.c_int32 * 2)()
    buf = C.create_string_buffer(2 * kf.CT_BYTES[k] + 2 * ctx.pk_bytes)
    for n in (0, -1):
        assert lib.kosk_registry_find(h, n, buf, slots) == -1 and lib.kosk_registry_enrol(h, n, buf, None, slots, buf) == -1
        assert lib.kosk_registry_enrol_verified(h, n, slots, buf) == -1 and lib.kosk_kem_enc_peers(h, n, buf, buf, buf, buf, buf) == -1
    assert lib.kosk_registry_find(h, 1, None, slots) == -1 and b"kosk_registry_find: invalid argument" in lib.kosk_last_error(h)
    assert lib.kosk_registry_find(h, 1, buf, None) == -1
    assert lib.kosk_registry_enrol(h, 1, None, None, slots, buf) == -1 and b"kosk_registry_enrol: invalid argument" in lib.kosk_last_error(h)
    assert lib.kosk_registry_enrol(h, 1, buf, None, None, buf) == -1 and lib.kosk_registry_enrol(h, 1, buf, None, slots, None) == -1
    assert lib.kosk_registry_enrol_verified(h, 1, None, buf) == -1 and b"kosk_registry_enrol_verified: invalid argument" in lib.kosk_last_error(h)
    assert lib.kosk_registry_enrol_verified(h, 1, slots, None) == -1
    assert lib.kosk_kem_enc_peers(h, 1, None, buf, buf, buf, buf) == -1 and b"kosk_kem_enc_peers: invalid argument" in lib.kosk_last_error(h)
    assert lib.kosk_kem_enc_peers(h, 1, buf, buf, None, buf, buf) == -1 and lib.kosk_kem_enc_peers(h, 1, buf, buf, buf, None, buf) == -1
    assert lib.kosk_kem_enc_peers(h, 1, buf, buf, buf, buf, None) == -1
    assert rc.counts(ctx, api) + ids(ctx, api) == before
    assert ctx.registry_enrol([pk]) == ([0], [rm.ADMITTED]) and ctx.registry_find([fp]) == [0]  # the handle still works
    ctx.close()


@pytest.mark.parametrize("k", KS)
def test_erasure(k, api):
    """8. after kosk_registry_enrol, kosk_registry_find, kosk_kem_enc_peers and the eviction no byte of the key, nor of its hash, is left
    in the handle's HBM; kosk_wipe_secrets and KOSK_WIPE_CALL leave the index alone"""
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(4)
    pk_a, pk_b = rc.pks(k)[3], rc.pks(k)[4]
    fa, fb = rm.fp(pk_a), rm.fp(pk_b)
    coins = list(rc.messages(k)[3:5])
    assert ctx.registry_enrol([pk_b, pk_a]) == ([0, 1], [rm.ADMITTED] * 2)
    assert ctx.secret_scan(pk_a[:64]) == 1 and ctx.secret_scan(fa) == 1  # in the slot, and nowhere else
    assert ctx.registry_enrol([pk_a]) == ([1], [rm.DUPLICATE]) and ctx.registry_find([fa, fb]) == [1, 0]
    enc = ctx.kem_enc_peers([fa, fb], coins)
    assert enc[2] == [True, True] and kf.sha3(enc[0][0]) == rc.items(k)[3]["ct"] and kf.sha3(enc[0][1]) == rc.items(k)[4]["ct"]
    assert ctx.secret_scan(pk_a[:64]) == 1 and ctx.secret_scan(fa) == 1
    rebuilds = ctx.path_count(api.Kosk.PATH_REGISTRY_INDEX)
    ctx.wipe_secrets()
    assert ctx.registry_find([fa, fb]) == [1, 0] and ctx.kem_enc_peers([fa, fb], coins) == enc
    ctx.set_wipe(api.WIPE_CALL)
    assert ctx.kem_enc_peers([fa, fb], coins) == enc and ctx.secret_scan(enc[1][0]) == 0 and ctx.secret_scan(coins[0]) == 0
    assert ctx.registry_find([fa, fb]) == [1, 0] and ctx.path_count(api.Kosk.PATH_REGISTRY_INDEX) == rebuilds
    ctx.set_wipe(api.WIPE_OFF)
    ctx.registry_evict([1])
    assert ctx.secret_scan(pk_a[:64]) == 0 and ctx.secret_scan(fa) == 0 and ctx.secret_scan(fb) == 1
    cts, sss, done = ctx.kem_enc_peers([fa, fb], coins)
    assert done == [False, True] and cts[0] == bytes(kf.CT_BYTES[k]) and sss[0] == bytes(32) and (cts[1], sss[1]) == (enc[0][1], enc[1][1])
    assert ctx.registry_find([fa]) == [-1] and ctx.secret_scan(fa) == 0 and ctx.secret_scan(pk_a[:64]) == 0
    ctx.close()


def test_neighbours(api, oracle, gpu_child):
    """9. kosk_kem_enc_verified, the fail masks, the one-key calls, the per-item calls and the bank level are the same before and after
    the new calls; so are kosk_kem_enc_slots, admit, evict and read (the comparisons of registry_cases); a handle that never calls the new
    functions has no index in its inventory; a cohort member, unmerged, in a fresh child process"""
    k = 3
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    pk3, sk3 = kf.keypair(k, 3)
    coins5 = list(rc.messages(k)[:5])
    tapes = [oracle.tape_bytes_for(k, 30 + i) for i in range(3)]
    pks, sks, pis = ctx.verifiable_keygen(tapes)
    bad = bytearray(pis[1]); bad[1000] ^= 1
    pis_t = [pis[0], bytes(bad), pis[2]]

    def neighbours():
        out = [ctx.kem_enc_verified(3, coins5[:3]), ctx.fail_masks(3), ctx.kem_enc_key(coins=coins5)]
        out.append(ctx.kem_dec_key(out[2][0]))
        out.append(ctx.kem_enc([pk3] * 5, coins5))
        out.append(ctx.kem_dec(out[4][0], [sk3] * 5))
        out.append((ctx.bank_level(), ctx.kem_key_state()))
        return out
    assert ctx.verify(pis_t, pks) == [True, False, True]
    ctx.kem_key_set(sk=sk3)
    first = neighbours()
    rc.admit_fixture(ctx, k)
    idx = [0, 97, 24, 2]
    slots = [rc.slot(i) for i in idx]
    enc0 = rc.check_enc(ctx, k, idx, slots)
    rc.check_read(ctx, k, idx, slots)
    assert neighbours() == first
    # the index is one more public buffer of the inventory, from the first lookup on: its empty entries are runs of 0xFF bytes
    assert ids(ctx, api) == (0, 0, 0)
    empty_run = b"\xff" * 32
    without = ctx.secret_scan(empty_run)
    assert ctx.registry_find(fps(k)) == [rc.slot(i) for i in range(kf.ITEMS)]
    assert ctx.secret_scan(empty_run) > without  # 1 024 entries, at most 130 of them taken: eight empty ones in a row somewhere
    assert neighbours() == first
    got = ctx.kem_enc_peers([fps(k)[i] for i in idx], [rc.messages(k)[i] for i in idx])
    assert got[:2] == enc0 and neighbours() == first
    assert ctx.registry_enrol_verified(3) == ([1, -1, 2], [rm.ADMITTED, rm.REJECTED, rm.ADMITTED])  # slot 0 holds fixture key 97
    assert neighbours() == first
    fresh = kf.keypair(k, 200)[0]  # pk3 is fixture key 3; slots 3 and 4 are occupied, 5 is the lowest empty one
    assert ctx.registry_enrol([pks[0], pk3, fresh]) == ([1, rc.slot(3), 5], [rm.DUPLICATE, rm.DUPLICATE, rm.ADMITTED]) and neighbours() == first
    # the existing calls on the same inputs, byte for byte
    assert rc.check_enc(ctx, k, idx, slots) == enc0
    rc.check_read(ctx, k, idx, slots)
    ctx.registry_evict([1, 2, 5])
    ctx.registry_admit([rc.pks(k)[0]], [rc.slot(0)])  # a replacement by the same key
    assert ctx.registry_level() == (kf.ITEMS, rc.CAPACITY)
    everyone = list(range(kf.ITEMS))
    rc.check_read(ctx, k, everyone, [rc.slot(i) for i in everyone])
    rc.check_enc(ctx, k, everyone, [rc.slot(i) for i in everyone])
    assert tuple(ctx.verifiable_keygen(tapes)) == (pks, sks, pis) and ctx.verify(pis_t, pks) == [True, False, True]
    assert neighbours() == first
    ctx.close()
    out = gpu_child("from tests.gpu_child_registry_index import cohort_member as f; f(2)")
    assert "cohort_member ok 2" in out


def test_registry_peers_example(torch_cuda):
    """10. examples/registry_peers 3 8 prints only lines ending in "= 1" """
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "registry_peers")
    if not os.path.exists(exe):
        pytest.fail("examples/registry_peers missing: run __graft_entry__.build()")
    r = subprocess.run([exe, "3", "8"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 7 and all(ln.endswith("= 1") for ln in lines), r.stdout
    assert lines[-1] == "[result] registry_peers success = 1"
