"""GPU tests of the context-bound proofs (format kosk-bind-v1; csrc/kosk_fs_kernels.hip: k_bind_values and the bound
instantiations of k_fs_chain).  References: hashlib for the kernels, and for whole proofs the CPU model that tests/bound_oracle.py derives
from the oracle (shared by the tests, computed once per process).  Every comparison is exact.  Multi-handle cases run in a child process."""
import ctypes as C
import hashlib
import os
import subprocess

import numpy as np
import pytest

from tests import bound_oracle as bo
from tests.test_bound_host import NOPEN, NPARTY, alpha_restated, opened_restated

pytestmark = pytest.mark.gpu

KS = (2, 3, 4)
SEL, SEL_WIN, SEL_OSORT, SEL_OPOS, NWIN = 1312, 160, 192, 352, 23
TABLE = NPARTY * 32


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return t


def _api():
    from mpcith_kyber_kosk_amd import api
    return api


def _dev(torch, arr):
    t = torch.from_numpy(np.ascontiguousarray(arr)).cuda()
    torch.cuda.synchronize()
    return t


def _first_diff(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), None)


def _ctxs(n, base=0):
    return [bo.context_of(base + b) for b in range(n)]


def _model(k, n, ctxs, first=0):
    rows = [bo.case(k, first + b, ctxs[b]) for b in range(n)]
    return [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]


def _assert_proofs(got, want, what):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g == w, (what, b, _first_diff(g, w))


# ---- k_bind_values
@pytest.mark.parametrize("k", KS)
def test_bind_values_against_hashlib(k, torch):
    """pk lengths 800 / 1184 / 1568 (last blocks of 120 / 96 / 72 bytes); n at and around a wave's worth; pk and contexts each from host
    and from device memory; context strides 32 and 40; the guard band behind n x 32 bytes stays as it was"""
    api = _api()
    ctx = api.Kosk(kyber_k=k, max_batch=1)
    rng = np.random.default_rng(1800 + k)
    for n in (1, 63, 64, 65):
        pks = rng.integers(0, 256, size=(n, ctx.pk_bytes), dtype=np.uint8)
        for pk_dev, ctx_dev, stride in ((False, False, 32), (True, True, 40), (False, True, 32), (True, False, 40)):
            cx = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
            want = [bo.bind_value(k, pks[b].tobytes(), cx[b, :32].tobytes()) for b in range(n)]
            d_pk, d_cx = _dev(torch, pks), _dev(torch, cx)
            d_out = torch.full(((n + 2) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.bind_device(n, d_pk.data_ptr() if pk_dev else pks.tobytes(), d_cx.data_ptr() if ctx_dev else cx.tobytes(), d_out.data_ptr(), stride)
            out = d_out.cpu().numpy()
            for b in range(n):
                assert out[32 * b:32 * b + 32].tobytes() == want[b], (k, n, pk_dev, ctx_dev, stride, b)
            assert (out[32 * n:] == 0xA5).all(), (k, n, "guard band")
    with pytest.raises(api.KoskError):
        ctx.bind_device(1, pks[0].tobytes(), bytes(32), d_out.data_ptr(), 31)
    with pytest.raises(api.KoskError):
        ctx.bind_device(1, pks[0].tobytes(), bytes(32), d_out.data_ptr() + 4)
    ctx.close()


# ---- the bound chain kernels
@pytest.mark.parametrize("stride", [TABLE, TABLE + 8])
@pytest.mark.parametrize("n", [1, 3])
def test_bound_chains_against_hashlib(n, stride, torch):
    api = _api()
    k = 3
    J = 70 + 2 * k
    ctx = api.Kosk(kyber_k=k, max_batch=1)
    rng = np.random.default_rng(1810 + n + stride)
    tables = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
    binds = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    d_t, d_b = _dev(torch, tables), _dev(torch, binds)
    tab = [tables[b, :TABLE].tobytes() for b in range(n)]
    for with_digest in (True, False):
        d_a = torch.full((n + 1, 80), -1, dtype=torch.int16, device="cuda")
        d_h = torch.zeros((n + 1, 32), dtype=torch.uint8, device="cuda")
        d_sel = torch.zeros((n + 1, SEL), dtype=torch.int16, device="cuda")
        d_rest = torch.zeros((n + 1, SEL), dtype=torch.int16, device="cuda")
        d_ch = torch.zeros((n + 1, 32), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        ctx.fs_alpha_bound_device(d_t.data_ptr(), stride, n, d_b.data_ptr(), d_a.data_ptr(), d_h.data_ptr() if with_digest else None)
        ctx.fs_opened_bound_device(d_t.data_ptr(), stride, n, d_b.data_ptr(), d_sel.data_ptr(), d_rest.data_ptr(), SEL, d_ch.data_ptr() if with_digest else None)
        ctx.synchronize()
        a, h = d_a.cpu().numpy().view(np.uint16), d_h.cpu().numpy()
        sel, rest, ch = d_sel.cpu().numpy().view(np.uint16), d_rest.cpu().numpy().view(np.uint16), d_ch.cpu().numpy()
        for b in range(n):
            wa, wh = alpha_restated(k, tab[b], binds[b].tobytes())
            assert a[b, :J].tolist() == wa and not a[b, J:].any(), (n, stride, b)
            wI, wrest, wch = opened_restated(tab[b], binds[b].tobytes())
            assert sel[b, :NOPEN].tolist() == wI and rest[b, :NPARTY - NOPEN].tolist() == wrest, (n, stride, b)
            assert sel[b, SEL_WIN:SEL_WIN + NWIN + 1].tolist() == [sum(1 for p in wrest if p < 64 * w) for w in range(NWIN + 1)]
            assert sel[b, SEL_OSORT:SEL_OSORT + NOPEN].tolist() == sorted(wI)
            assert sel[b, SEL_OPOS:SEL_OPOS + NOPEN].tolist() == [wI.index(p) for p in sorted(wI)]
            if with_digest:
                assert h[b].tobytes() == wh and ch[b].tobytes() == wch
            else:
                assert not h[b].any() and not ch[b].any()
        assert (a[n] == 0xFFFF).all() and not h[n].any() and not sel[n].any() and not rest[n].any() and not ch[n].any()  # guard rows
    # the unbound entry points on the same tables still give the unbound values
    d_a = torch.zeros((n, 80), dtype=torch.int16, device="cuda")
    d_sel = torch.zeros((n, SEL), dtype=torch.int16, device="cuda")
    d_rest = torch.zeros((n, SEL), dtype=torch.int16, device="cuda")
    d_h = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.fs_alpha_device(d_t.data_ptr(), stride, n, d_a.data_ptr(), d_h.data_ptr())
    ctx.fs_opened_device(d_t.data_ptr(), stride, n, d_sel.data_ptr(), d_rest.data_ptr(), SEL)
    ctx.synchronize()
    a, sel, h = d_a.cpu().numpy().view(np.uint16), d_sel.cpu().numpy().view(np.uint16), d_h.cpu().numpy()
    for b in range(n):
        wa, wh = alpha_restated(k, tab[b])
        assert a[b, :J].tolist() == wa and h[b].tobytes() == wh and sel[b, :NOPEN].tolist() == opened_restated(tab[b])[0]
    with pytest.raises(api.KoskError):
        ctx.fs_alpha_bound_device(d_t.data_ptr(), stride, n, d_b.data_ptr() + 4, d_a.data_ptr())
    ctx.close()


# ---- bound proofs, byte for byte the derived model's
@pytest.mark.parametrize("fs", [0, 1])
@pytest.mark.parametrize("k", KS)
def test_bound_proofs_equal_the_model(k, fs, oracle, torch):
    """verifiable_keygen on 3 tapes under 3 distinct contexts, max_batch = 3; then prove_keys on the secret keys it returned, with the same
    tapes and contexts: the same bytes (INTEGRATION.md 9's rule, armed)"""
    api = _api()
    n = 3
    tapes = [oracle.tape_bytes_for(k, b) for b in range(n)]
    ctxs = _ctxs(n)
    wpk, wsk, wpi = _model(k, n, ctxs)
    ctx = api.Kosk(kyber_k=k, max_batch=n, fs_mode=fs)
    ctx.set_contexts(ctxs)
    pks, sks, pis = ctx.verifiable_keygen(tapes)
    assert pks == wpk and sks == wsk
    _assert_proofs(pis, wpi, ("keygen", k, fs))
    got, ok = ctx.prove_keys(sks, tapes)
    assert ok == [True] * n
    _assert_proofs(got, wpi, ("prove_keys", k, fs))
    assert ctx.verify(pis, pks) == [True] * n
    ctx.close()


@pytest.mark.parametrize("fs", [0, 1])
def test_seeded_compact_and_resident_forms(fs, oracle, torch):
    api = _api()
    k, n = 3, 3
    tapes = [oracle.tape_bytes_for(k, b) for b in range(n)]
    ctxs = _ctxs(n)
    wpk, wsk, wpi = _model(k, n, ctxs)
    ctx = api.Kosk(kyber_k=k, max_batch=n, fs_mode=fs)
    d_cx = _dev(torch, np.frombuffer(b"".join(c + bytes(8) for c in ctxs), np.uint8).copy())
    ctx.set_contexts(d_cx.data_ptr(), n=n, stride=40)  # armed from device memory, stride 40
    # compact
    pks, sks, blobs = ctx.verifiable_keygen_compact(tapes)
    assert pks == wpk and sks == wsk
    for b in range(n):
        img = C.create_string_buffer(ctx.proof_bytes)
        assert api.lib.kosk_proof_decompress(k, blobs[b], img) == 0
        assert img.raw == wpi[b], ("compact", fs, b, _first_diff(img.raw, wpi[b]))
    ok = C.create_string_buffer(n)
    assert api.lib.kosk_verify_batch_compact(ctx.handle, n, b"".join(blobs), b"".join(pks), ok) == 0 and ok.raw == b"\x01" * n
    # resident, then the resident verifier on the keys it left in HBM
    ctx.verifiable_keygen_resident(tapes)
    assert ctx.keys(n) == (wpk, wsk)
    _assert_proofs(ctx.fetch_proofs(n), wpi, ("resident", fs))
    assert ctx.verify_resident_pk(n) == [True] * n
    assert ctx.verify_resident_pk(n, pks) == [True] * n
    # staged prover inputs + prove_resident
    ctx.stage_prover_inputs(tapes)
    ctx.prove_resident(n)
    _assert_proofs(ctx.fetch_proofs(n), wpi, ("staged", fs))
    # seeded: the model on the tapes of the seeds
    seeds = [hashlib.sha3_256(b"kosk-bind-test-seed:%d" % b).digest() for b in range(n)]
    rows = [bo.verifiable_keygen(k, api.tape_from_seed(k, s), context=ctxs[b]) for b, s in enumerate(seeds)]
    spk, ssk, spi = ctx.verifiable_keygen(seeds=seeds)
    assert spk == [r[0] for r in rows] and ssk == [r[1] for r in rows]
    _assert_proofs(spi, [r[2] for r in rows], ("seeded", fs))
    ctx.stage_verifier_inputs(spi, spk)
    assert ctx.verify_resident(n) == [True] * n
    ctx.close()


@pytest.mark.parametrize("fs", [0, 1])
def test_contexts_follow_the_chunks(fs, oracle, torch):
    """5 proofs on a max_batch = 2 handle: position b of the whole call uses context b, for the prover and for the verifier"""
    api = _api()
    k, n = 2, 5
    tapes = [oracle.tape_bytes_for(k, b) for b in range(n)]
    ctxs = _ctxs(n)
    wpk, wsk, wpi = _model(k, n, ctxs)
    ctx = api.Kosk(kyber_k=k, max_batch=2, fs_mode=fs)
    ctx.set_contexts(ctxs)
    pks, sks, pis = ctx.verifiable_keygen(tapes)
    assert pks == wpk and sks == wsk
    _assert_proofs(pis, wpi, ("chunked", fs))
    assert ctx.verify(pis, pks) == [True] * n
    got, ok = ctx.prove_keys(sks, tapes)
    assert ok == [True] * n
    _assert_proofs(got, wpi, ("chunked prove_keys", fs))
    moved = ctxs[1:] + ctxs[:1]
    ctx.set_contexts(moved)
    assert ctx.verify(pis, pks) == [False] * n
    ctx.close()


@pytest.mark.parametrize("fs", [0, 1])
def test_two_streams(fs, oracle, torch):
    api = _api()
    k, n = 2, 3
    tapes = [oracle.tape_bytes_for(k, b) for b in range(n)]
    ctxs = _ctxs(n)
    wpk, wsk, wpi = _model(k, n, ctxs)
    ctx = api.Kosk(kyber_k=k, max_batch=n, fs_mode=fs, streams=2)
    assert ctx.streams == 2
    ctx.set_contexts(ctxs)
    pks, sks, pis = ctx.verifiable_keygen(tapes)
    assert pks == wpk and sks == wsk
    _assert_proofs(pis, wpi, ("streams", fs))
    assert ctx.verify(pis, pks) == [True] * n
    ctx.verifiable_keygen_resident(tapes)
    _assert_proofs(ctx.fetch_proofs(n), wpi, ("streams resident", fs))
    assert ctx.verify_resident_pk(n) == [True] * n
    ctx.close()


# ---- the verifier
def _flip(c, byte, bit):
    return c[:byte] + bytes([c[byte] ^ (1 << bit)]) + c[byte + 1:]


@pytest.mark.parametrize("fs", [0, 1])
@pytest.mark.parametrize("k", KS)
def test_verifier_bits_equal_the_model(k, fs, oracle, torch):
    api = _api()
    n = 3
    ctxs = _ctxs(n)
    pks, _, pis = _model(k, n, ctxs)
    plain = [oracle.verifiable_keygen(k, oracle.tape_bytes_for(k, b))[2] for b in range(n)]
    ctx = api.Kosk(kyber_k=k, max_batch=n, fs_mode=fs)

    def both(armed, proofs):
        """the handle's bits under `armed` (None: disarmed) and the model's"""
        if armed is None:
            ctx.clear_contexts()
        else:
            ctx.set_contexts(armed)
        got = ctx.verify(proofs, pks)
        want = [bo.verify(k, proofs[b], pks[b], context=None if armed is None else armed[b]) for b in range(n)]
        assert got == want, (k, fs, got, want)
        return got
    assert both(ctxs, pis) == [True] * n
    assert both([_flip(ctxs[0], 0, 0), _flip(ctxs[1], 31, 7), ctxs[2]], pis) == [False, False, True]
    assert both(None, pis) == [False] * n            # bound proofs on a disarmed handle
    assert both(None, plain) == [True] * n
    assert both(ctxs, plain) == [False] * n          # unbound proofs on an armed handle
    assert both([ctxs[2], ctxs[1], ctxs[0]], pis) == [False, True, False]
    # the resident verifier paths give the same bits, and the KEM encapsulates to the accepted position only
    ctx.stage_verifier_inputs(pis, pks)
    assert ctx.verify_resident(n) == [False, True, False]
    coins = [hashlib.sha3_256(b"kosk-bind-test-coins:%d" % b).digest() for b in range(n)]
    cts, sss, done = ctx.kem_enc_verified(n, coins)
    assert done == [False, True, False]
    ct1, ss1 = ctx.kem_enc([pks[1]], [coins[1]])
    assert cts[1] == ct1[0] and sss[1] == ss1[0] and any(cts[1])
    for b in (0, 2):
        assert not any(cts[b]) and not any(sss[b])
    ctx.close()


# ---- arming and disarming
def test_arming_rules(oracle, torch):
    api = _api()
    k = 2
    tape = oracle.tape_bytes_for(k, 0)
    ctx = api.Kosk(kyber_k=k, max_batch=2)
    ctx.set_contexts(_ctxs(1))
    pks, sks, pis = ctx.verifiable_keygen([tape])
    assert pis[0] == bo.case(k, 0, _ctxs(1)[0])[2]
    for call in (lambda: ctx.verifiable_keygen([tape, tape]), lambda: ctx.verify(pis * 2, pks * 2), lambda: ctx.verifiable_keygen_resident([tape, tape]),
                 lambda: ctx.prove_keys(sks * 2, [tape, tape]), lambda: ctx.verify_resident_pk(2, pks * 2)):
        with pytest.raises(api.KoskError, match="armed with fewer contexts"):
            call()
    inst, rnd, rng = (bytes(getattr(api.lib, f)(k)) for f in ("kosk_mlwe_inst_bytes", "kosk_randomness_bytes", "kosk_range_proof_bytes"))
    with pytest.raises(api.KoskError, match="armed handle"):
        ctx.verify_inst(pis, [inst])
    with pytest.raises(api.KoskError, match="armed handle"):
        ctx.prove_prepared([inst], [rnd], [rng], [tape])
    with pytest.raises(api.KoskError, match="context_stride"):
        ctx.set_contexts(_ctxs(1), stride=31)
    assert ctx.verify(pis, pks) == [True]               # the refused calls changed nothing: still armed with the one context
    ctx.clear_contexts()
    opk, osk, opi, _, _ = oracle.verifiable_keygen(k, tape)
    assert ctx.verifiable_keygen([tape]) == ([opk], [osk], [opi])  # arm -> disarm: the plain oracle's bytes again
    assert ctx.verify([opi], [opk]) == [True] and ctx.verify(pis, pks) == [False]
    ctx.clear_contexts()                                 # disarming twice is harmless
    ctx.close()


def test_armed_member_of_a_cohort(torch, gpu_child):
    """tests/gpu_child_bound.py: cohort_armed_member"""
    out = gpu_child("from tests.gpu_child_bound import cohort_armed_member; cohort_armed_member()")
    assert "cohort_armed_member ok 2" in out


@pytest.mark.parametrize("k", KS)
def test_enrol_bound_example(k, torch):
    """examples/enrol_bound.cpp on the C ABI: challenge -> bound proofs for existing keys -> bound verify -> kosk_kem_enc_verified ->
    decapsulation; the replay under new nonces and the disarmed verifier accept nothing"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "enrol_bound")
    if not os.path.exists(exe):
        pytest.fail("examples/enrol_bound missing: run __graft_entry__.build()")
    r = subprocess.run([exe, str(k), "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "[enrol] kyber_k %d: 3 bound proofs, 3 accepted, 3 shared secrets agree" % k in r.stdout
    assert "[enrol] replay under new nonces: 0 accepted; on a disarmed handle: 0 accepted" in r.stdout
    assert "[result] enrol_bound success" in r.stdout
