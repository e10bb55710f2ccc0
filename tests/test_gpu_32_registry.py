"""GPU tests of the verified-key registry (include/kosk_mi355x.h: kosk_registry_reserve, _level, _admit_verified, _admit, _evict, _read,
kosk_kem_enc_slots) against tests/golden/kem_vectors_v1.json -- what the reference's crypto_kem_enc_derand returned
for 130 distinct keys --, against the per-item calls on the same handle, which tests/test_gpu_14_kem.py pins to that fixture, and against
hashlib for H(pk).  Every comparison is exact.  Handles use max_batch = 3 unless a case verifies proofs: the KEM calls do not depend on it."""
import ctypes as C
import hashlib
import os
import subprocess

import pytest

from tests import kem_fixture as kf
from tests import registry_cases as rc

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


@pytest.mark.parametrize("n", (1, 3, 65, 130))
@pytest.mark.parametrize("k", KS)
def test_enc_slots_equals_the_reference(k, n, handles):
    """1. every ct digest and ss of kosk_kem_enc_slots on the first n fixture items against the fixture, done all 1; the registry holds
    the pk bytes as given (item 2: the non-canonical encoding) and hashlib's SHA3-256 of them"""
    ctx = handles[k]
    idx = list(range(n))
    slots = [rc.slot(i) for i in idx]
    rc.check_enc(ctx, k, idx, slots)
    rc.check_read(ctx, k, idx, slots)


@pytest.mark.parametrize("k", KS)
def test_enc_slots_equals_the_per_item_call(k, handles):
    """2. 67 items over 5 slots in a repeating, unsorted order -- equal slots within one wave and across waves -- against kosk_kem_enc_batch
    of the corresponding pk list"""
    ctx = handles[k]
    keys = [97, 2, 24, 5, 11]  # slot 0, the non-canonical key, slot 299, two in between
    order = [keys[(3 * b + b // 5) % 5] for b in range(67)]
    assert len(set(order[:5])) == 5 and order[:5] != sorted(order[:5])
    coins = [hashlib.shake_256(b"registry-per-item:%d:%d" % (k, b)).digest(32) for b in range(67)]
    cts, sss, done = ctx.kem_enc_slots([rc.slot(i) for i in order], coins)
    assert done == [True] * 67
    assert (cts, sss) == ctx.kem_enc([rc.pks(k)[i] for i in order], coins)


@pytest.mark.parametrize("n", (1, 64, 65, rc.WAVE_MAX, rc.WAVE_MAX + 1))
def test_admission_layout_edges(n, api):
    """3. admissions of one key, a whole wave, one past it, the largest on the wave layout and the smallest on the per-lane layout
    (keys modulo 130, capacity 1 100): every slot read back against hashlib, the first, the 1 024th and the 1 025th slot encapsulated to"""
    k = 3
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(rc.EDGE_CAPACITY)
    idx = [b % kf.ITEMS for b in range(n)]
    slots = [rc.edge_slot(b) for b in range(n)]
    ctx.registry_admit([rc.pks(k)[i] for i in idx], slots)
    assert ctx.registry_level() == (n, rc.EDGE_CAPACITY) and ctx.path_count(api.Kosk.PATH_REGISTRY_ADMIT) == 1
    rc.check_read(ctx, k, idx, slots)
    probe = [b for b in (0, rc.WAVE_MAX - 1, rc.WAVE_MAX) if b < n]
    rc.check_enc(ctx, k, [idx[b] for b in probe], [slots[b] for b in probe])
    # every slot that was not named is still empty
    named = set(slots)
    rest = [s for s in range(rc.EDGE_CAPACITY) if s not in named]
    states, got_pk, got_h = ctx.registry_read(rest)
    assert states == [0] * len(rest) and set(got_pk) == {bytes(ctx.pk_bytes)} and set(got_h) == {bytes(32)}
    ctx.close()


def test_per_lane_admission_on_small_batches(torch_cuda, gpu_child):
    """3. KOSK_DEBUG_KEM_WAVE_MAX=0: n = 3 and 65 on the per-lane layout"""
    out = gpu_child("from tests.gpu_child_registry import per_lane_admission as f; f(3)", env={"KOSK_DEBUG_KEM_WAVE_MAX": "0"})
    assert "per_lane_admission ok 3" in out


def test_launch_groups(api, torch_cuda):
    """4. one admission of 16 385 keys and one kosk_kem_enc_slots of 16 385 items, two launch groups each: positions 0, 16 383 and 16 384
    against the fixture (an offset into `slots` that restarts at a launch group puts item 16 384 on key 0's slot)"""
    k, n = 3, rc.CHUNK + 1
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(rc.BIG_CAPACITY)
    idx = [b % kf.ITEMS for b in range(n)]
    slots = [rc.big_slot(b) for b in range(n)]
    torch = torch_cuda
    blob = b"".join(rc.pks(k))  # the 130 records over and over, in device memory
    d_pk = torch.frombuffer(bytearray(blob * (n // kf.ITEMS + 1))[:n * ctx.pk_bytes], dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    ctx.registry_admit(d_pk.data_ptr(), slots, n=n)
    assert ctx.registry_level() == (n, rc.BIG_CAPACITY) and ctx.path_count(api.Kosk.PATH_REGISTRY_ADMIT) == 2
    cts, sss, done = ctx.kem_enc_slots(slots, [rc.messages(k)[i] for i in idx])
    assert done == [True] * n and ctx.path_count(api.Kosk.PATH_KEM_ENC_SLOTS) == 2
    want = rc.items(k)
    for b in (0, rc.CHUNK - 1, rc.CHUNK):
        assert kf.sha3(cts[b]) == want[idx[b]]["ct"] and sss[b].hex() == want[idx[b]]["ss"], b
    probe = [0, rc.CHUNK - 1, rc.CHUNK]
    rc.check_read(ctx, k, [idx[b] for b in probe], [slots[b] for b in probe])
    ctx.registry_evict(slots)
    assert ctx.registry_level() == (0, rc.BIG_CAPACITY)
    ctx.close()


def _verified_handle(api, oracle, k, first_tape):
    """a handle whose last verify call covered three proofs, proof 1 tampered: bits [1, 0, 1]"""
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    pks, sks, pis = ctx.verifiable_keygen([oracle.tape_bytes_for(k, first_tape + i) for i in range(3)])
    bad = bytearray(pis[1]); bad[1000] ^= 1
    pis = [pis[0], bytes(bad), pis[2]]
    assert ctx.verify(pis, pks) == [True, False, True]
    return ctx, pks, sks, pis


def test_admit_verified(api, oracle):
    """5. the keys of a verify call with bits [1, 0, 1] into slots [5, 0, 2]: done is those bits, `used` goes up by 2, slot 0 keeps the
    key it had; on a fresh handle kosk_kem_enc_slots on those slots equals kosk_kem_enc_verified byte for byte"""
    k = 2
    coins = [hashlib.shake_256(b"registry-verified:%d" % i).digest(32) for i in range(3)]
    ctx, pks, sks, pis = _verified_handle(api, oracle, k, 40)
    ctx.registry_reserve(8)
    other = rc.pks(k)[7]
    ctx.registry_admit([other], [0])
    assert ctx.registry_level() == (1, 8)
    assert ctx.registry_admit_verified([5, 0, 2]) == [True, False, True]
    assert ctx.registry_level() == (3, 8) and ctx.path_count(api.Kosk.PATH_REGISTRY_ADMIT) == 2
    states, got_pk, got_h = ctx.registry_read([5, 0, 2, 1])
    assert states == [1, 1, 1, 0] and got_pk[:3] == [pks[0], other, pks[2]] and got_pk[3] == bytes(ctx.pk_bytes)
    assert got_h[:3] == [hashlib.sha3_256(p).digest() for p in (pks[0], other, pks[2])]
    cts, sss, done = ctx.kem_enc_slots([5, 0, 2], coins)
    assert done == [True] * 3 and (cts, sss) == ctx.kem_enc([pks[0], other, pks[2]], coins)
    assert ctx.kem_dec([cts[0], cts[2]], [sks[0], sks[2]]) == [sss[0], sss[2]]
    ctx.close()
    ctx, pks, sks, pis = _verified_handle(api, oracle, k, 40)
    ctx.registry_reserve(8)
    assert ctx.registry_admit_verified([5, 0, 2]) == [True, False, True] and ctx.registry_level() == (2, 8)
    got = ctx.kem_enc_slots([5, 0, 2], coins)
    assert got == ctx.kem_enc_verified(3, coins)
    assert got[2] == [True, False, True] and got[0][1] == bytes(kf.CT_BYTES[k]) and got[1][1] == bytes(32)
    ctx.close()


def test_admit_verified_refusals(api, oracle, gpu_child):
    """5. every refusal of kosk_registry_admit_verified: -1, the call's name, level and counters unchanged"""
    k = 2
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(8)
    tapes = [oracle.tape_bytes_for(k, 40 + i) for i in range(3)]

    def refused(text, slots=(5, 0, 2)):
        before = rc.counts(ctx, api)
        with pytest.raises(api.KoskError, match="kosk_registry_admit_verified: .*" + text):
            ctx.registry_admit_verified(list(slots))
        assert rc.counts(ctx, api) == before
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
    assert ctx.registry_admit_verified([5, 0, 2]) == [True] * 3 and ctx.registry_level() == (3, 8)  # the handle still works
    ctx.close()
    out = gpu_child("from tests.gpu_child_registry import cohort_member as f; f(2)")
    assert "cohort_member ok 2" in out
    out = gpu_child("from tests.gpu_child_registry import admit_verified_refused_with_two_streams as f; f(2)")
    assert "admit_verified_refused_with_two_streams ok 2" in out


@pytest.mark.parametrize("k", KS)
def test_replace_evict_scan_wipe(k, api, handles):
    """6. key A, then key B in one slot: the ciphertexts follow the key, `used` stays; after the eviction done = 0, zero outputs, an empty
    record, and no byte of the key left in the handle's HBM; the wipes leave the registry alone and clear the call's scratch.  (The per-item
    call this is compared with runs on ANOTHER handle: it leaves its pk records in its workspace, where the scan would find them.)"""
    ctx, ref = api.Kosk(kyber_k=k, max_batch=3), handles[k]
    ctx.registry_reserve(4)
    pk_a, pk_b, pk_c = rc.pks(k)[3], rc.pks(k)[4], rc.pks(k)[5]
    coins = list(rc.messages(k)[3:5])
    assert ctx.secret_scan(pk_a[:32]) == 0
    ctx.registry_admit([pk_a, pk_c], [2, 0])
    assert ctx.registry_level() == (2, 4) and ctx.secret_scan(pk_a[:32]) == 1  # in the slot, and nowhere else
    enc_a = ctx.kem_enc_slots([2, 2], coins)
    assert enc_a[:2] == ref.kem_enc([pk_a] * 2, coins)
    assert kf.sha3(enc_a[0][0]) == rc.items(k)[3]["ct"]
    ctx.registry_admit([pk_b], [2])
    assert ctx.registry_level() == (2, 4) and ctx.secret_scan(pk_a[:32]) == 0
    enc_b = ctx.kem_enc_slots([2, 2], coins)
    assert enc_b[:2] == ref.kem_enc([pk_b] * 2, coins) and enc_b != enc_a
    assert kf.sha3(enc_b[0][1]) == rc.items(k)[4]["ct"]
    # the wipe leaves level, read and the bytes of kosk_kem_enc_slots unchanged
    read0 = ctx.registry_read([0, 1, 2, 3])
    assert read0[0] == [1, 0, 1, 0] and read0[1][2] == pk_b
    ctx.wipe_secrets()
    assert ctx.registry_level() == (2, 4) and ctx.registry_read([0, 1, 2, 3]) == read0 and ctx.kem_enc_slots([2, 2], coins) == enc_b
    # the per-call scratch is secret: mode off keeps a returned ss, KOSK_WIPE_CALL does not
    assert ctx.secret_scan(enc_b[1][0]) >= 1
    ctx.set_wipe(api.WIPE_CALL)
    assert ctx.kem_enc_slots([2, 2], coins) == enc_b and ctx.secret_scan(enc_b[1][0]) == 0 and ctx.secret_scan(coins[0]) == 0
    assert ctx.registry_level() == (2, 4) and ctx.registry_read([0, 1, 2, 3]) == read0
    ctx.set_wipe(api.WIPE_OFF)
    ctx.wipe_secrets()
    # the eviction
    assert ctx.secret_scan(pk_b[:32]) >= 1 and ctx.secret_scan(pk_c[:32]) >= 1
    ctx.registry_evict([2, 2, 1])  # a repeat and an empty slot are fine
    assert ctx.registry_level() == (1, 4)
    assert ctx.secret_scan(pk_b[:32]) == 0 and ctx.secret_scan(pk_c[:32]) >= 1
    cts, sss, done = ctx.kem_enc_slots([2, 0], coins)
    assert done == [False, True] and cts[0] == bytes(kf.CT_BYTES[k]) and sss[0] == bytes(32)
    assert (cts[1], sss[1]) == tuple(x[0] for x in ref.kem_enc([pk_c], coins[1:]))
    assert ctx.registry_read([2]) == ([0], [bytes(ctx.pk_bytes)], [bytes(32)])
    # an empty registry may be reserved again, a non-empty one not; reserve(0) frees
    with pytest.raises(api.KoskError, match="kosk_registry_reserve: .*not empty"):
        ctx.registry_reserve(8)
    ctx.registry_evict([0])
    ctx.registry_reserve(8)
    assert ctx.registry_level() == (0, 8) and ctx.secret_scan(pk_c[:32]) == 0
    ctx.registry_reserve(0)
    assert ctx.registry_level() == (0, 0)
    ctx.close()


@pytest.mark.parametrize("k", KS)
def test_explicit_admission(k, api, torch_cuda):
    """7. accept with a zero in the middle, accept = None, pk records in device memory; the non-canonical pk (item 2) and an all-0xFFF
    t-hat against kosk_kem_enc_batch on the same bytes"""
    torch = torch_cuda
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(rc.CAPACITY)
    all_fff = b"\xff" * (384 * k) + rc.pks(k)[0][-32:]
    keys = [rc.pks(k)[2], all_fff, rc.pks(k)[9]]
    coins = [hashlib.shake_256(b"registry-explicit:%d:%d" % (k, b)).digest(32) for b in range(3)]
    want = ctx.kem_enc(keys, coins)
    ctx.registry_admit(keys, [299, 150, 0], accept=[1, 0, 1])
    assert ctx.registry_level() == (2, rc.CAPACITY)
    cts, sss, done = ctx.kem_enc_slots([299, 150, 0], coins)
    assert done == [True, False, True] and cts[1] == bytes(kf.CT_BYTES[k]) and sss[1] == bytes(32)
    assert (cts[0], sss[0], cts[2], sss[2]) == (want[0][0], want[1][0], want[0][2], want[1][2])
    assert kf.sha3(want[0][0]) != rc.items(k)[2]["ct"]  # other coins than the fixture's: the parity is test 1's
    ctx.registry_admit(keys, [299, 150, 0])  # accept = None: all three, two of them replacements
    assert ctx.registry_level() == (3, rc.CAPACITY)
    assert ctx.kem_enc_slots([299, 150, 0], coins) == (want[0], want[1], [True] * 3)
    assert ctx.registry_read([150])[1:] == ([all_fff], [hashlib.sha3_256(all_fff).digest()])
    d_pk = torch.frombuffer(bytearray(b"".join(keys)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    ctx.registry_admit(d_pk.data_ptr(), [7, 8, 9], accept=[0, 1, 1], n=3)
    assert ctx.registry_level() == (5, rc.CAPACITY)
    assert ctx.kem_enc_slots([9, 8], coins[:2]) == tuple(list(x) for x in ctx.kem_enc([keys[2], keys[1]], coins[:2])) + ([True, True],)
    assert ctx.registry_read([7, 8, 9])[0] == [0, 1, 1] and bytes(d_pk.cpu().numpy()) == b"".join(keys)
    ctx.close()


def test_device_buffers(handles, torch_cuda):
    """8. coins, ct, ss and done in device memory (torch), K = 3, n = 65, a sentinel around every output, nothing outside them written"""
    torch = torch_cuda
    k, n, pad = 3, 65, 64
    ctx = handles[k]
    ctb = kf.CT_BYTES[k]
    coins = list(rc.messages(k)[:n])
    slots = [rc.slot(i) for i in range(n)]
    d_m = torch.frombuffer(bytearray(b"".join(coins)), dtype=torch.uint8).cuda()
    d_ct = torch.full((pad + n * ctb + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_ss = torch.full((pad + n * 32 + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_done = torch.full((pad + n + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.kem_enc_slots(slots, coins=d_m.data_ptr(), out=(d_ct.data_ptr() + pad, d_ss.data_ptr() + pad, d_done.data_ptr() + pad))
    ct, ss, done = bytes(d_ct.cpu().numpy()), bytes(d_ss.cpu().numpy()), bytes(d_done.cpu().numpy())
    for buf in (ct, ss, done):
        assert buf[:pad] == bytes([SENTINEL]) * pad and buf[-pad:] == bytes([SENTINEL]) * pad
    assert done[pad:-pad] == b"\x01" * n
    want = rc.items(k)
    for b in range(n):
        assert kf.sha3(ct[pad + ctb * b:pad + ctb * (b + 1)]) == want[b]["ct"] and ss[pad + 32 * b:pad + 32 * b + 32].hex() == want[b]["ss"]
    assert bytes(d_m.cpu().numpy()) == b"".join(coins)


@pytest.mark.parametrize("k", KS)
def test_coins_from_the_randombytes_callback(k, handles):
    """9. coins=None with an empty slot among 7: exactly 7 draws of 32 bytes, in item order, whatever done says; the results equal the
    explicit call on what the callback returned"""
    ctx = handles[k]
    empty = 1  # slot(i) = 1 has no solution below 130: 37 i = -10 mod 300 needs i = 170
    assert empty not in [rc.slot(i) for i in range(kf.ITEMS)]
    slots = [rc.slot(0), rc.slot(1), rc.slot(97), empty, rc.slot(24), rc.slot(0), rc.slot(2)]
    calls = []

    def rb(nbytes):
        out = hashlib.shake_256(b"registry-callback:%d:%d" % (k, len(calls))).digest(nbytes)
        calls.append(out)
        return out
    ctx.set_randombytes(rb)
    try:
        got = ctx.kem_enc_slots(slots)
    finally:
        ctx.set_randombytes(None)
    assert [len(c) for c in calls] == [32] * 7
    assert got == ctx.kem_enc_slots(slots, calls) and len(calls) == 7
    assert got[2] == [True, True, True, False, True, True, True] and got[0][3] == bytes(kf.CT_BYTES[k]) and got[1][3] == bytes(32)
    keys = [0, 1, 97, 24, 0, 2]
    want = ctx.kem_enc([rc.pks(k)[i] for i in keys], calls[:3] + calls[4:])
    assert (got[0][:3] + got[0][4:], got[1][:3] + got[1][4:]) == want


def test_refusals(api):
    """10. each returns -1 with the call's name and starts nothing: counters and level unchanged"""
    k = 3
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    lib, h = api.lib, ctx.handle
    pk = rc.pks(k)[0]
    coins = [rc.messages(k)[0]]

    def refused(name, text, fn):
        before = rc.counts(ctx, api)
        with pytest.raises(api.KoskError, match="kosk_%s: .*%s" % (name, text)):
            fn()
        assert rc.counts(ctx, api) == before
    # no registry reserved
    assert ctx.registry_level() == (0, 0)
    refused("registry_admit", "no registry is reserved", lambda: ctx.registry_admit([pk], [0]))
    refused("registry_admit_verified", "no registry is reserved", lambda: ctx.registry_admit_verified([0]))
    refused("registry_evict", "no registry is reserved", lambda: ctx.registry_evict([0]))
    refused("registry_read", "no registry is reserved", lambda: ctx.registry_read([0]))
    refused("kem_enc_slots", "no registry is reserved", lambda: ctx.kem_enc_slots([0], coins))
    refused("registry_reserve", "capacity < 0", lambda: ctx.registry_reserve(-1))
    ctx.registry_reserve(4)
    ctx.registry_admit([pk], [1])
    # a slot id of -1 and of `capacity`
    for bad in (-1, 4):
        refused("registry_admit", r"outside \[0, capacity\)", lambda: ctx.registry_admit([pk, pk], [0, bad]))
        refused("registry_admit_verified", r"outside \[0, capacity\)", lambda: ctx.registry_admit_verified([bad]))
        refused("registry_evict", r"outside \[0, capacity\)", lambda: ctx.registry_evict([1, bad]))
        refused("registry_read", r"outside \[0, capacity\)", lambda: ctx.registry_read([1, bad]))
        refused("kem_enc_slots", r"outside \[0, capacity\)", lambda: ctx.kem_enc_slots([bad], coins))
    # a repeated id in an admission, whatever accept says
    refused("registry_admit", "named twice", lambda: ctx.registry_admit([pk, pk], [2, 2]))
    refused("registry_admit", "named twice", lambda: ctx.registry_admit([pk, pk, pk], [2, 3, 2], accept=[1, 1, 0]))
    refused("registry_admit_verified", "named twice", lambda: ctx.registry_admit_verified([3, 3]))
    # a refused kosk_kem_enc_slots draws no coin
    calls = []
    ctx.set_randombytes(lambda nbytes: calls.append(nbytes) or bytes(nbytes))
    try:
        refused("kem_enc_slots", r"outside \[0, capacity\)", lambda: ctx.kem_enc_slots([1, 4]))
    finally:
        ctx.set_randombytes(None)
    assert calls == []
    # reserve while occupied, reserve(-1)
    refused("registry_reserve", "not empty", lambda: ctx.registry_reserve(8))
    refused("registry_reserve", "capacity < 0", lambda: ctx.registry_reserve(-1))
    # n < 1 and NULL pointers on the C ABI
    before = rc.counts(ctx, api)
    slots = (C.c_int32 * 2)(1, 2)
    buf = C.create_string_buffer(2 * kf.CT_BYTES[k] + 2 * ctx.pk_bytes)
    for n in (0, -1):
        for name, rcode in (("kosk_registry_admit", lib.kosk_registry_admit(h, n, buf, None, slots)),
                            ("kosk_registry_admit_verified", lib.kosk_registry_admit_verified(h, n, slots, buf)),
                            ("kosk_registry_evict", lib.kosk_registry_evict(h, n, slots)),
                            ("kosk_registry_read", lib.kosk_registry_read(h, n, slots, buf, None, None)),
                            ("kosk_kem_enc_slots", lib.kosk_kem_enc_slots(h, n, slots, buf, buf, buf, buf))):
            assert rcode == -1, (name, n)
    assert lib.kosk_kem_enc_slots(h, 1, slots, buf, None, buf, buf) == -1 and b"kosk_kem_enc_slots: invalid argument" in lib.kosk_last_error(h)
    assert lib.kosk_kem_enc_slots(h, 1, slots, buf, buf, None, buf) == -1 and lib.kosk_kem_enc_slots(h, 1, slots, buf, buf, buf, None) == -1
    assert lib.kosk_kem_enc_slots(h, 1, None, buf, buf, buf, buf) == -1
    assert lib.kosk_registry_admit(h, 1, None, None, slots) == -1 and b"kosk_registry_admit: invalid argument" in lib.kosk_last_error(h)
    assert lib.kosk_registry_admit(h, 1, buf, None, None) == -1
    assert lib.kosk_registry_admit_verified(h, 1, slots, None) == -1 and b"kosk_registry_admit_verified: invalid argument" in lib.kosk_last_error(h)
    assert lib.kosk_registry_read(h, 1, slots, None, None, None) == -1 and b"kosk_registry_read: invalid argument" in lib.kosk_last_error(h)
    assert lib.kosk_registry_evict(h, 1, None) == -1 and b"kosk_registry_evict: invalid argument" in lib.kosk_last_error(h)
    assert rc.counts(ctx, api) == before
    assert ctx.registry_read([1]) == ([1], [pk], [hashlib.sha3_256(pk).digest()])  # the key admitted at the start is still there
    ctx.close()


def test_neighbours(api, oracle):
    """11. the one-key calls, kosk_kem_enc_batch / _dec_batch, kosk_kem_enc_verified, a key generation and a verify call return the same
    before, between and after the registry calls; a workspace growth leaves the registry intact"""
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
        return out
    assert ctx.verify(pis_t, pks) == [True, False, True]
    ctx.kem_key_set(sk=sk3)
    first = neighbours()
    assert first[0][2] == [True, False, True] and first[2] == first[4] and first[3] == first[5] == first[2][1]
    ctx.registry_reserve(rc.CAPACITY)
    assert neighbours() == first
    ctx.registry_admit(list(rc.pks(k)), [rc.slot(i) for i in range(kf.ITEMS)])
    assert neighbours() == first
    assert not {1, 2, 6} & {rc.slot(i) for i in range(kf.ITEMS)}  # three slots the fixture's keys leave empty
    assert ctx.registry_admit_verified([1, 2, 6]) == [True, False, True]
    assert neighbours() == first
    rc.check_enc(ctx, k, [0, 97, 24], [rc.slot(0), rc.slot(97), rc.slot(24)])
    assert neighbours() == first
    ctx.registry_evict([1, 6])
    ctx.registry_read([0, 1])
    assert neighbours() == first
    assert ctx.kem_key_state() == api.KEM_KEY_SK and ctx.bank_level() == (0, 0)
    assert tuple(ctx.verifiable_keygen(tapes)) == (pks, sks, pis) and ctx.verify(pis_t, pks) == [True, False, True]
    opk, osk, opi, _, _ = oracle.verifiable_keygen(k, tapes[0])
    assert (pks[0], sks[0], pis[0]) == (opk, osk, opi)
    assert neighbours() == first
    # a per-item call of 1 025 items after the small ones frees and reallocates the KEM workspace, not the registry
    grown = ctx.kem_enc([rc.pks(k)[b % kf.ITEMS] for b in range(1025)], [rc.messages(k)[b % kf.ITEMS] for b in range(1025)])
    assert kf.sha3(grown[0][1024]) == rc.items(k)[1024 % kf.ITEMS]["ct"]
    assert ctx.registry_level() == (kf.ITEMS, rc.CAPACITY)
    idx = list(range(kf.ITEMS))
    rc.check_read(ctx, k, idx, [rc.slot(i) for i in idx])
    rc.check_enc(ctx, k, idx, [rc.slot(i) for i in idx])
    ctx.close()


def test_cohort_member_and_block_limit(torch_cuda, gpu_child):
    """11. in child processes: a cohort member admits explicitly and encapsulates by slot (with test 5's refusal); with
    KOSK_DEBUG_XOF_BLOCKS=1 an admission returns "block limit" and leaves its slots empty"""
    out = gpu_child("from tests.gpu_child_registry import block_limit_leaves_the_slots_empty as f; f(3)", env={"KOSK_DEBUG_XOF_BLOCKS": "1"})
    assert "block_limit_leaves_the_slots_empty ok 3" in out


def test_registry_enrol_example(torch_cuda):
    """12. examples/registry_enrol 3 8 prints only lines ending in "= 1" """
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "registry_enrol")
    if not os.path.exists(exe):
        pytest.fail("examples/registry_enrol missing: run __graft_entry__.build()")
    r = subprocess.run([exe, "3", "8"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 6 and all(ln.endswith("= 1") for ln in lines), r.stdout
    assert lines[-1] == "[result] registry_enrol success = 1"
