"""GPU tests of the erasure calls (csrc/kosk_wipe.hip: k_wipe, k_scan; kosk_wipe_secrets, kosk_set_wipe,
kosk_secret_scan, kosk_wipe_device).  The needles and the calls that plant them are in tests/wipe_cases.py.  Every comparison is exact.
max_batch <= 3, KEM calls of 3 items: the row matrix is a few tens of MB and a scan takes milliseconds."""
import os
import subprocess

import numpy as np
import pytest

from tests import wipe_cases as wc

pytestmark = pytest.mark.gpu

KS = wc.KS


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return t


def _api():
    from mpcith_kyber_kosk_amd import api
    return api


def _hits(ctx, needles):
    return {n.name: ctx.secret_scan(n.data) for n in needles}


def _all_gone(ctx, needles, what):
    h = _hits(ctx, needles)
    assert not any(h.values()), (what, {k: v for k, v in h.items() if v})


def _all_there(ctx, needles, what):
    h = _hits(ctx, needles)
    assert all(v >= 1 for v in h.values()), (what, {k: v for k, v in h.items() if v < 1})


# ---- cases 1 and 2: the scan sees what is there; after kosk_wipe_secrets it is gone and the public state is not
@pytest.mark.parametrize("k", KS + (4,))
def test_scan_finds_every_needle_and_the_wipe_removes_it(k, torch):
    api = _api()
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    planted = []
    pk0 = None
    for plant in wc.GROUND_TRUTH:
        needles, res = plant(ctx)
        _all_there(ctx, needles, plant.__name__)  # mode off, right behind the call that planted them
        planted += needles
        if plant is wc.plant_keygen_tapes:
            pk0 = res[0][0]
    # the public key of the first key generation was replaced in d_pk since; one that is resident now is the control
    ctx.verifiable_keygen_resident([wc.tape(k, 70 + b) for b in range(2)])
    pks, sks = ctx.keys(2)
    planted += wc.sk_needles(sks[1]) + wc.tape_needles(wc.tape(k, 71))
    ctl = wc.control(pks[0])
    assert ctx.secret_scan(ctl.data) >= 1 and pk0 is not None
    assert ctx.secret_scan(bytes(range(100, 132))) == 0  # a needle that nobody planted
    before = ctx.path_count(api.Kosk.PATH_WIPE)
    ctx.wipe_secrets()
    assert ctx.path_count(api.Kosk.PATH_WIPE) > before
    _all_gone(ctx, planted, "after kosk_wipe_secrets")
    assert ctx.secret_scan(ctl.data) >= 1
    # needles of 16 and 64 bytes, and the lengths the call refuses
    assert ctx.secret_scan(pks[0][:16]) >= 1 and ctx.secret_scan(pks[0][:64]) >= 1
    for bad in (15, 65, 0):
        with pytest.raises(api.KoskError):
            ctx.secret_scan(pks[0][:bad])
    ctx.close()


@pytest.mark.parametrize("k", KS)
def test_public_resident_state_survives_the_wipe(k, torch):
    api = _api()
    n = 3
    tapes = [wc.tape(k, 80 + b) for b in range(n)]
    coins = [wc.coins32(10 + b) for b in range(n)]
    ctx, twin = api.Kosk(kyber_k=k, max_batch=n), api.Kosk(kyber_k=k, max_batch=n)
    for h in (ctx, twin):
        h.verifiable_keygen_resident(tapes)
    pis = ctx.fetch_proofs(n)
    dig = [torch.as_tensor(ctx.resident_digests(r, n), device="cuda").cpu().numpy().tobytes() for r in (0, 1)]
    ctx.wipe_secrets()
    assert ctx.fetch_proofs(n) == pis == twin.fetch_proofs(n)
    assert [torch.as_tensor(ctx.resident_digests(r, n), device="cuda").cpu().numpy().tobytes() for r in (0, 1)] == dig
    assert ctx.verify_resident_pk(n) == twin.verify_resident_pk(n) == [True] * n
    assert ctx.fail_masks(n) == twin.fail_masks(n)
    ctx.wipe_secrets()
    assert ctx.fail_masks(n) == twin.fail_masks(n)
    assert ctx.kem_enc_verified(n, coins=coins) == twin.kem_enc_verified(n, coins=coins)
    # a tampered resident proof: the same bits and masks after a wipe as without one
    bad = list(pis)
    flip = bytearray(bad[1]); flip[api.proof_field(k, 0)[0] + 7] ^= 1; bad[1] = bytes(flip)
    pks, _sks = ctx.keys(n)
    for h in (ctx, twin):
        h.stage_verifier_inputs(bad, pks)
    ctx.wipe_secrets()
    assert ctx.verify_resident_pk(n) == twin.verify_resident_pk(n) == [True, False, True]
    assert ctx.fail_masks(n) == twin.fail_masks(n) and ctx.fail_masks(n)[1] != 0
    # staged inputs that were wiped are not proven over
    for stage in (lambda: ctx.stage_prover_inputs(tapes), lambda: wc.stage_keys(ctx, 2)):
        stage()
        ctx.wipe_secrets()
        with pytest.raises(api.KoskError, match="staged inputs were wiped"):
            ctx.prove_resident(2)
    ctx.stage_prover_inputs(tapes)
    ctx.prove_resident(n)
    assert ctx.fetch_proofs(n) == pis
    ctx.close(); twin.close()


# ---- case 3: a wiped handle is a fresh handle
def _flow(ctx, k, n, armed):
    api = _api()
    if armed:
        ctx.set_contexts([wc.context(b) for b in range(n)])
    tapes = [wc.tape(k, 90 + b) for b in range(n)]
    pks, sks, pis = ctx.verifiable_keygen(tapes)
    out = [pks, sks, pis, ctx.verify(pis, pks), ctx.fail_masks(n)]
    pis2, ok = ctx.prove_keys(sks, tapes=[wc.tape(k, 95 + b) for b in range(n)])
    packed = [api.dense_pack(k, p) for p in pis2]
    assert all(rc == 0 for rc, _rec in packed)
    out += [pis2, ok, ctx.verify_dense([rec for _rc, rec in packed], pks), ctx.fail_masks(n)]
    coins = [wc.coins32(20 + b) for b in range(n)]
    cts, sss = ctx.kem_enc(pks, coins=coins)
    out += [cts, sss, ctx.kem_dec(cts, sks), ctx.kem_enc_verified(n, coins=coins)]
    assert out[3] == [True] * n and out[7] == [True] * n and out[11] == sss
    return out


@pytest.mark.parametrize("armed", [False, True])
@pytest.mark.parametrize("fs", [0, 1])
@pytest.mark.parametrize("k", KS)
def test_a_wiped_handle_is_a_fresh_handle(k, fs, armed, torch):
    api = _api()
    n = 2
    used = api.Kosk(kyber_k=k, max_batch=n, fs_mode=fs)
    for plant in (wc.plant_keygen_seeded, wc.plant_prove_keys_derived, wc.plant_kem_keypair, wc.plant_kem_dec):
        plant(used)
    used.verify_resident_pk(n)  # the verifier's workspace has been through a call too
    used.wipe_secrets()
    fresh = api.Kosk(kyber_k=k, max_batch=n, fs_mode=fs)
    a, b = _flow(used, k, n, armed), _flow(fresh, k, n, armed)
    for i, (x, y) in enumerate(zip(a, b)):
        assert x == y, (k, fs, armed, "step", i)
    used.close(); fresh.close()


# ---- case 4: KOSK_WIPE_CALL
@pytest.mark.parametrize("k", KS)
def test_wipe_call_mode_every_entry_point(k, torch):
    api = _api()
    mb = 2
    w, off = api.Kosk(kyber_k=k, max_batch=mb), api.Kosk(kyber_k=k, max_batch=mb)
    for bad in (2, -1, 7):
        with pytest.raises(api.KoskError):
            w.set_wipe(bad)
    needles, _ = wc.plant_keygen_tapes(w)
    _all_there(w, needles, "a refused mode changed nothing")
    w.set_wipe(api.WIPE_CALL)
    launches = w.path_count(api.Kosk.PATH_WIPE)
    for plant in wc.WIPE_CALL_PLANTS:
        needles, res = plant(w)
        _all_gone(w, needles, plant.__name__)
        assert w.path_count(api.Kosk.PATH_WIPE) > launches, plant.__name__
        launches = w.path_count(api.Kosk.PATH_WIPE)
        _n, want = plant(off)
        assert res == want, plant.__name__
    # the entry points that write to device memory of the caller: the results are the caller's and stay, the handle's copies go
    seeds = [wc.seed(30 + b) for b in range(mb)]
    d_tapes = torch.zeros((mb, (w.tape_bytes + 7) // 8 * 8), dtype=torch.uint8, device="cuda")
    w.tape_expand_device(seeds, d_tapes.data_ptr(), d_tapes.shape[1])
    assert [bytes(r[:w.tape_bytes]) for r in d_tapes.cpu().numpy()] == [api.tape_from_seed(k, s) for s in seeds]
    _all_gone(w, [wc.Needle("seed", seeds[-1])] + wc.tape_needles(api.tape_from_seed(k, seeds[-1])), "tape_expand_device")
    _pks, sks = wc.honest_keys(k, mb)
    d_seeds = torch.zeros((mb * 32,), dtype=torch.uint8, device="cuda")
    w.keyseed_device(mb, b"".join(sks), d_seeds.data_ptr())
    assert d_seeds.cpu().numpy().tobytes() == b"".join(api.keyseed_value(k, s) for s in sks)
    _all_gone(w, wc.sk_needles(sks[-1]) + [wc.Needle("derived seed", api.keyseed_value(k, sks[-1]))], "keyseed_device")
    # device tapes read in place are the caller's: proven from, never touched
    tp = [wc.tape(k, 100 + b) for b in range(mb)]
    stride = (w.tape_bytes + 63) // 64 * 64
    host = np.zeros((mb, stride), np.uint8)
    for b in range(mb):
        host[b, :w.tape_bytes] = np.frombuffer(tp[b], np.uint8)
    d_tp = torch.from_numpy(host).cuda()
    torch.cuda.synchronize()
    w.verifiable_keygen_resident(d_tp.data_ptr(), n=mb, tape_stride=stride)
    assert (d_tp.cpu().numpy() == host).all()
    _all_gone(w, wc.tape_needles(tp[-1]) + wc.sk_needles(w.keys(mb)[1][-1]), "device tapes read in place")
    # after a staging call the needles are still there; after the kosk_prove_resident that follows they are gone
    needles, ok = wc.stage_keys(w)
    _all_there(w, needles, "staging call under WIPE_CALL")
    w.prove_resident(2)
    _all_gone(w, needles, "prove_resident after the staging call")
    # a chunked call: n = 2 max_batch + 1, every chunk's secrets are gone and the results are the plain handle's
    needles, res = wc.plant_keygen_tapes(w, n=2 * mb + 1, first=110)
    _all_gone(w, needles + wc.tape_needles(wc.tape(k, 110)) + wc.sk_needles(res[1][0]) + wc.sk_needles(res[1][mb]), "chunked call")
    assert res == wc.plant_keygen_tapes(off, n=2 * mb + 1, first=110)[1]
    # back to off: nothing is wiped behind a call any more
    w.set_wipe(api.WIPE_OFF)
    needles, _ = wc.plant_kem_keypair(w)
    _all_there(w, needles, "mode off again")
    w.close(); off.close()


# ---- case 5: k_wipe writes inside its regions and nowhere else
LENGTHS = (0, 1, 15, 16, 17, 255, 4096 + 3, (1 << 20) + 5)
OFFSETS = (0, 1, 8, 15)


@pytest.mark.parametrize("k", [2, 4])  # (k_wipe does not depend on K; the handle's stream and counters do exist per handle)
def test_wipe_device_bounds(k, torch):
    api = _api()
    ctx = api.Kosk(kyber_k=k, max_batch=1)
    guard = 256
    for length in LENGTHS:
        for off in OFFSETS:
            buf = torch.full((guard + 16 + length + guard,), 0xA5, dtype=torch.uint8, device="cuda")
            assert buf.data_ptr() % 256 == 0
            torch.cuda.synchronize()
            start = guard + off
            ctx.wipe_device([buf.data_ptr() + start], [length])
            got = buf.cpu().numpy()
            assert not got[start:start + length].any(), (length, off, "inside")
            assert (got[:start] == 0xA5).all() and (got[start + length:] == 0xA5).all(), (length, off, "guards")
    # 40 regions of mixed sizes and alignments in one call (one launch), 64 guard bytes between neighbours
    sizes = [LENGTHS[i % 7] + (i % 3) for i in range(40)]
    starts, pos = [], 64
    for i, s in enumerate(sizes):
        pos += OFFSETS[i % 4]
        starts.append(pos)
        pos += s + 64 + (-(pos + s) % 16)
    buf = torch.full((pos,), 0xA5, dtype=torch.uint8, device="cuda")
    want = np.full((pos,), 0xA5, np.uint8)
    for st, s in zip(starts, sizes):
        want[st:st + s] = 0
    torch.cuda.synchronize()
    before = ctx.path_count(api.Kosk.PATH_WIPE)
    ctx.wipe_device([buf.data_ptr() + st for st in starts], sizes)
    assert ctx.path_count(api.Kosk.PATH_WIPE) == before + 1
    assert (buf.cpu().numpy() == want).all()
    # more regions than one launch carries, and refused arguments
    many = [8 + i for i in range(100)]
    buf = torch.full((100 * 128,), 0xA5, dtype=torch.uint8, device="cuda")
    want = np.full((100 * 128,), 0xA5, np.uint8)
    for i, s in enumerate(many):
        want[128 * i + 3:128 * i + 3 + s] = 0
    torch.cuda.synchronize()
    ctx.wipe_device([buf.data_ptr() + 128 * i + 3 for i in range(100)], many)
    assert (buf.cpu().numpy() == want).all()
    # the size from which a single run is handed to the runtime's fill instead of k_wipe (320 MiB), next to a small region in the same
    # call; checked where it lies, nothing of it crosses PCIe
    big = (320 << 20) + 5
    buf = torch.full((256 + 1 + big + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    small = torch.full((256 + 17 + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = ctx.path_count(api.Kosk.PATH_WIPE)
    ctx.wipe_device([buf.data_ptr() + 257, small.data_ptr() + 256], [big, 17])
    assert ctx.path_count(api.Kosk.PATH_WIPE) == before + 1  # the small region's launch
    assert not bool(buf[257:257 + big].any()) and bool((buf[:257] == 0xA5).all()) and bool((buf[257 + big:] == 0xA5).all())
    got = small.cpu().numpy()
    assert not got[256:273].any() and (got[:256] == 0xA5).all() and (got[273:] == 0xA5).all()
    del buf
    host = np.full((64,), 0xA5, np.uint8)
    with pytest.raises(api.KoskError):
        ctx.wipe_device([host.ctypes.data], [64])
    assert (host == 0xA5).all()
    ctx.wipe_device([], [])
    ctx.close()


# ---- several handles and lane threads at once: in a fresh child process (tests/gpu_child_wipe.py)
def test_cohort_member_in_wipe_call_mode(gpu_child, torch):
    out = gpu_child("from tests.gpu_child_wipe import cohort_member_wipes_its_own_block; cohort_member_wipes_its_own_block(3)", timeout=300)
    assert "cohort_member_wipes_its_own_block ok" in out


def test_wipe_call_mode_with_two_streams(gpu_child, torch):
    out = gpu_child("from tests.gpu_child_wipe import two_streams; two_streams(3)", timeout=300)
    assert "two_streams ok" in out


def test_wipe_call_mode_on_an_error_return(gpu_child, torch):
    out = gpu_child("from tests.gpu_child_wipe import error_path; error_path(3)", timeout=300)
    assert "error_path ok" in out


@pytest.mark.parametrize("k", KS)
def test_wipe_audit_example(k, torch):
    """examples/wipe_audit.cpp on the C ABI: key generation, prove_keys, a KEM round trip, the scan before and after a wipe, KOSK_WIPE_CALL"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "wipe_audit")
    if not os.path.exists(exe):
        pytest.fail("examples/wipe_audit missing: run __graft_entry__.build()")
    r = subprocess.run([exe, str(k), "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 7 and all(ln.endswith("= 1") for ln in lines), r.stdout
    assert lines[-1] == "[result] wipe_audit success = 1"
