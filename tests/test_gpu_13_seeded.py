"""GPU tests of seeded proving (include/kosk_mi355x.h, format kosk-seedtape-v1): k_tape_expand against hashlib byte for byte, the
seeded entry points against the explicit-tape calls on hashlib tapes, the one-seed-per-proof callback sequence and the per-handle
entropy mode, merged cohorts with mixed randomness sources, argument errors, graph replay.  Every comparison is exact."""
import ctypes as C

import pytest

from tests.gpu_child_seeded import device_rows, hashlib_tape, seed_for

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return torch


@pytest.mark.parametrize("k", [2, 3, 4])
def test_tape_expand_kernel_every_byte_against_hashlib(k, torch_cuda):
    """kosk_tape_expand_device: every byte of every tape equals the hashlib construction, for n in {1, 2, 46, 47, 277}, seeds in host
    and in device memory at strides 32 and 64, tape strides T rounded up to 8, to 64, and (T rounded up to 8) + 4096 -- the
    interface takes multiples of 8 only.  The buffers are pre-filled with a sentinel that must survive everywhere outside
    [b * stride, b * stride + T), in front of the first tape and behind the last one included.  The tightest stride is also run from a
    base that is 8 but not 0 mod 16."""
    import numpy as np
    from mpcith_kyber_kosk_amd import api
    torch = torch_cuda
    ctx = api.Kosk(kyber_k=k, max_batch=277)
    T = ctx.tape_bytes
    t8, t64 = (T + 7) // 8 * 8, (T + 63) // 64 * 64
    strides = [t8, t64, t8 + 4096]
    seeds = [seed_for(k, i, "kernel") for i in range(277)]
    tapes = np.stack([np.frombuffer(hashlib_tape(k, s), np.uint8) for s in seeds])
    before = ctx.path_counts()["tape_expand"]
    calls = 0
    for n in (1, 2, 46, 47, 277):
        variants = [(dev, ss) for dev in (False, True) for ss in (32, 64)]
        combos = [(v, st) for v in variants for st in strides] if n < 277 else [(variants[i], strides[i % 3]) for i in range(4)]
        for (dev, ss), stride in combos:
            lead = 72 if stride == t8 else 64  # base = 8 mod 16 for the tightest stride
            buf = torch.full((lead + n * stride + 64,), SENTINEL, dtype=torch.uint8, device="cuda")
            keep = None
            if dev:
                keep = device_rows(torch, seeds[:n], ss)
                src = keep.data_ptr()
            else:
                src = [s for s in seeds[:n]] if ss == 32 else None
            torch.cuda.synchronize()
            if dev:
                ctx.tape_expand_device(src, buf.data_ptr() + lead, stride, n=n, seed_stride=ss)
            elif ss == 32:
                ctx.tape_expand_device(src, buf.data_ptr() + lead, stride)
            else:  # host seeds 64 bytes apart (raw call: the Python wrapper packs lists at 32)
                blob = b"".join(s + b"\xee" * 32 for s in seeds[:n])
                rc = api.lib.kosk_tape_expand_device(ctx.handle, n, C.c_char_p(blob), 64, C.c_void_p(buf.data_ptr() + lead), stride)
                assert rc == 0, api.lib.kosk_last_error(ctx.handle)
            calls += 1
            got = buf.cpu().numpy()
            want = np.full(got.shape, SENTINEL, np.uint8)
            body = want[lead:lead + n * stride].reshape(n, stride)
            body[:, :T] = tapes[:n]
            if not np.array_equal(got, want):
                bad = np.nonzero(got != want)[0]
                pytest.fail("k %d n %d device seeds %s seed_stride %d tape stride %d: %d bytes differ, first at buffer offset %d "
                            "(tape %d byte %d)" % (k, n, dev, ss, stride, len(bad), bad[0], (bad[0] - lead) // stride, (bad[0] - lead) % stride))
            del buf, keep
    assert ctx.path_counts()["tape_expand"] == before + calls
    ctx.close()


@pytest.mark.parametrize("fs", [0, 1])
@pytest.mark.parametrize("k", [2, 3, 4])
def test_seeded_calls_equal_explicit_tape_calls(k, fs, oracle, torch_cuda):
    """Every seeded entry point returns pk, sk and proofs byte-identical, at every position, to the existing explicit-tape call on the
    hashlib tapes of the same seeds: resident + fetch, batch with n = 46, batch above max_batch on a handle with streams = 2, the
    compact batch, and the staged form + prove_resident; host and device Fiat-Shamir.  Every proof verifies; positions 0, 23 and the
    last are also compared with the CPU oracle."""
    from mpcith_kyber_kosk_amd import api
    n = 46
    seeds = [seed_for(k, i, "pipeline%d" % fs) for i in range(n)]
    tapes = [hashlib_tape(k, s) for s in seeds]
    assert tapes[0] == api.tape_from_seed(k, seeds[0])
    ctx = api.Kosk(kyber_k=k, max_batch=n, fs_mode=fs)
    want = ctx.verifiable_keygen(tapes)  # the existing explicit-tape call
    for b in (0, 23, n - 1):
        opk, osk, opi, _, _ = oracle.verifiable_keygen(k, tapes[b])
        assert (want[0][b], want[1][b], want[2][b]) == (opk, osk, opi), ("oracle", b)
    assert ctx.verify(want[2], want[0]) == [True] * n
    before = ctx.path_counts()["tape_expand"]
    # resident + fetch
    assert ctx.verifiable_keygen_resident(seeds=seeds) == n
    assert ctx.keys(n) == want[:2], "seeded_resident keys"
    assert ctx.verify_resident_pk(n) == [True] * n
    assert ctx.fetch_proofs(n) == want[2], "seeded_resident proofs"
    # seeds in device memory, 64 bytes apart
    dev = device_rows(torch_cuda, seeds, 64)
    ctx.verifiable_keygen_resident(seeds=dev.data_ptr(), n=n, seed_stride=64)
    assert ctx.keys(n) == want[:2] and ctx.fetch_proofs(n) == want[2], "seeded_resident, device seeds"
    # batch, n = 46
    got = ctx.verifiable_keygen(seeds=seeds)
    assert got == want, "seeded_batch"
    assert ctx.verify(got[2], got[0]) == [True] * n
    # staged form + prove_resident
    ctx.stage_prover_inputs(seeds=seeds)
    assert ctx.keys(n) == want[:2], "stage_prover_inputs_seeded keys"
    ctx.prove_resident(n)
    assert ctx.fetch_proofs(n) == want[2], "stage_prover_inputs_seeded + prove_resident"
    # compact batch
    cwant = ctx.verifiable_keygen_compact(tapes)
    cgot = ctx.verifiable_keygen_compact(seeds=seeds)
    assert cgot == cwant and cgot[:2] == want[:2], "seeded_batch_compact"
    assert ctx.path_counts()["tape_expand"] == before + 5
    ctx.close()
    # n above max_batch, two streams: chunks of 20 dealt to two sub-contexts
    small = api.Kosk(kyber_k=k, max_batch=20, streams=2, fs_mode=fs)
    assert small.verifiable_keygen(tapes) == want, "explicit tapes, chunked"
    assert small.verifiable_keygen(seeds=seeds) == want, "seeded_batch above max_batch, streams = 2"
    assert small.verifiable_keygen_compact(seeds=seeds) == cwant, "seeded_batch_compact above max_batch, streams = 2"
    small.stage_prover_inputs(seeds=seeds[:20])  # split over the two sub-contexts
    small.prove_resident(20)
    assert small.keys(20) == (want[0][:20], want[1][:20]) and small.fetch_proofs(20) == want[2][:20]
    small.verifiable_keygen_resident(seeds=seeds[3:22])
    assert small.fetch_proofs(19) == want[2][3:22]
    small.close()


@pytest.mark.parametrize("streams", [1, 2])
def test_callback_sees_one_seed_per_proof_and_entropy_mode(streams, oracle, torch_cuda):
    """seeds == NULL: the recording callback sees exactly n calls of 32 bytes, in proof order, and the outputs equal the seeded call on
    the recorded seeds.  After kosk_set_entropy(KOSK_ENTROPY_SEED) the EXISTING entry points with tapes = None do the same.  On a
    fresh handle, and after the mode is set back to 0, the callback sees the reference's 64, M x 32, nfresh x 302 per proof."""
    from mpcith_kyber_kosk_amd import api
    k, n = 3, 5
    p = oracle.params(k)
    calls, data = [], []
    counter = [0]

    def rb(nbytes):
        calls.append(nbytes)
        counter[0] += 1
        import hashlib
        out = hashlib.shake_256(b"callback:%d" % counter[0]).digest(nbytes)
        data.append(out)
        return out

    def reset():
        del calls[:], data[:]
    ctx = api.Kosk(kyber_k=k, max_batch=3, streams=streams)  # n > max_batch: the batch calls chunk
    big = api.Kosk(kyber_k=k, max_batch=n, streams=streams)
    ctx.set_randombytes(rb)
    big.set_randombytes(rb)
    per_proof = [64] + [32] * p.M + [302] * (p.tape_calls - 1 - p.M)  # 64, M x 32, nfresh x 302
    assert sum(per_proof) == p.tape_bytes

    def check_reference_sequence(h, note):
        reset()
        pks, sks, pis = h.verifiable_keygen(None, n=2)
        assert calls == per_proof * 2, note
        tape = [b"".join(data[i * len(per_proof):(i + 1) * len(per_proof)]) for i in range(2)]
        assert (pks[0], sks[0], pis[0]) == oracle.verifiable_keygen(k, tape[0])[:3], note
        assert h.verify(pis, pks) == [True, True]
    check_reference_sequence(ctx, "fresh handle")

    def check_seeded(h, fn, m, note):
        """fn() makes a call that draws through the callback and returns (pks, sks, pis)"""
        reset()
        got = fn()
        assert calls == [32] * m, (note, calls[:8], len(calls))
        drawn = list(data)
        reset()
        again = h.verifiable_keygen(seeds=drawn)
        assert not calls and again == got, note
        assert got == tuple(h.verifiable_keygen([hashlib_tape(k, s) for s in drawn])), note
        return got

    def resident(h, m, **kw):
        h.verifiable_keygen_resident(n=m, **kw)
        return h.keys(m) + (h.fetch_proofs(m),)

    def staged(h, m, **kw):
        h.stage_prover_inputs(n=m, **kw)
        h.prove_resident(m)
        return h.keys(m) + (h.fetch_proofs(m),)
    # the seeded entry points with seeds == NULL
    check_seeded(ctx, lambda: tuple(ctx.verifiable_keygen(seeds=True, n=n)), n, "seeded_batch, seeds NULL")
    check_seeded(big, lambda: resident(big, n, seeds=True), n, "seeded_resident, seeds NULL")
    check_seeded(big, lambda: staged(big, n, seeds=True), n, "stage_prover_inputs_seeded, seeds NULL")
    reset()
    cg = ctx.verifiable_keygen_compact(seeds=True, n=n)
    assert calls == [32] * n and cg == ctx.verifiable_keygen_compact(seeds=list(data)[:n])
    check_reference_sequence(ctx, "default mode after seeded calls")
    # the per-handle mode: the EXISTING entry points with tapes = None
    for h in (ctx, big):
        h.set_entropy(api.ENTROPY_SEED)
    check_seeded(ctx, lambda: tuple(ctx.verifiable_keygen(None, n=n)), n, "keygen_batch in seed mode")
    check_seeded(big, lambda: resident(big, n), n, "keygen_resident in seed mode")
    check_seeded(big, lambda: staged(big, n), n, "stage_prover_inputs in seed mode")
    reset()
    cg = ctx.verifiable_keygen_compact(None, n=n)
    assert calls == [32] * n and cg == ctx.verifiable_keygen_compact(seeds=list(data)[:n])
    # explicit tapes in seed mode: unchanged
    tp = [oracle.tape_bytes_for(k, 7)]
    reset()
    assert ctx.verifiable_keygen(tp)[2][0] == oracle.verifiable_keygen(k, tp[0])[2] and not calls
    # a constructor keyword does the same as the setter
    kw = api.Kosk(kyber_k=k, max_batch=2, entropy=api.ENTROPY_SEED)
    kw.set_randombytes(rb)
    check_seeded(kw, lambda: tuple(kw.verifiable_keygen(None, n=2)), 2, "entropy= keyword")
    kw.close()
    # back to the default: the reference's sequence again
    for h in (ctx, big):
        h.set_entropy(api.ENTROPY_TAPE)
    check_reference_sequence(ctx, "mode set back to 0")
    check_reference_sequence(big, "mode set back to 0")
    # OS entropy, seeded: proofs verify and differ
    ctx.set_randombytes(None)
    pks, sks, pis = ctx.verifiable_keygen(seeds=True, n=2)
    assert ctx.verify(pis, pks) == [True, True] and pis[0] != pis[1] and pks[0] != pks[1]
    ctx.close()
    big.close()


@pytest.mark.parametrize("fs", [0, 1])
def test_cohorts_with_mixed_randomness_sources(fs, torch_cuda, gpu_child):
    """tests/gpu_child_seeded.py: seeded_cohorts -- six caller threads, combine = 6, K = 3, 46 proofs each: three seeded callers (one of
    them a ragged n = 17), two with in-place device tapes, one with host tapes; each member's bytes equal its unmerged call."""
    out = gpu_child("from tests.gpu_child_seeded import seeded_cohorts; seeded_cohorts(%d)" % fs)
    assert "seeded_cohorts ok fs %d all_seeded 0" % fs in out


@pytest.mark.parametrize("fs", [0, 1])
def test_cohorts_all_seeded(fs, torch_cuda, gpu_child):
    out = gpu_child("from tests.gpu_child_seeded import seeded_cohorts; seeded_cohorts(%d, all_seeded=True)" % fs)
    assert "seeded_cohorts ok fs %d all_seeded 1" % fs in out


def test_argument_errors_leave_the_handle_usable(oracle, torch_cuda):
    """seed_stride = 16, an odd d_tapes base, n = 0 and n > max_batch on the resident form, entropy modes other than 0 / 1: rc -1, an
    error text, nothing started -- and the handle works afterwards.  (Argument errors only.)"""
    from mpcith_kyber_kosk_amd import api
    lib = api.lib
    k, mb = 2, 4
    ctx = api.Kosk(kyber_k=k, max_batch=mb)
    seeds = [seed_for(k, i, "errors") for i in range(mb)]
    blob = b"".join(seeds)
    pk = C.create_string_buffer(ctx.pk_bytes * (mb + 1)); sk = C.create_string_buffer(ctx.sk_bytes * (mb + 1))
    pi = C.create_string_buffer(ctx.proof_bytes * mb)

    def refused(rc):
        assert rc == -1
        assert len(lib.kosk_last_error(ctx.handle)) > 0
    before = ctx.path_counts()["tape_expand"]
    refused(lib.kosk_verifiable_keygen_seeded_resident(ctx.handle, 2, C.c_char_p(blob), 16, pk, sk))
    refused(lib.kosk_verifiable_keygen_seeded_batch(ctx.handle, 2, C.c_char_p(blob), 16, pk, sk, pi))
    refused(lib.kosk_verifiable_keygen_seeded_batch_compact(ctx.handle, 2, C.c_char_p(blob), 16, pk, sk, pi))
    refused(lib.kosk_stage_prover_inputs_seeded(ctx.handle, 2, C.c_char_p(blob), 16, pk, sk))
    refused(lib.kosk_verifiable_keygen_seeded_resident(ctx.handle, 0, C.c_char_p(blob), 32, pk, sk))
    refused(lib.kosk_verifiable_keygen_seeded_resident(ctx.handle, mb + 1, C.c_char_p(blob), 32, pk, sk))
    refused(lib.kosk_verifiable_keygen_seeded_resident(ctx.handle, 2, C.c_char_p(blob), 32, None, sk))
    stride = (ctx.tape_bytes + 7) // 8 * 8
    buf = torch_cuda.full((mb * stride + 64,), SENTINEL, dtype=torch_cuda.uint8, device="cuda")
    torch_cuda.cuda.synchronize()
    refused(lib.kosk_tape_expand_device(ctx.handle, 2, C.c_char_p(blob), 32, C.c_void_p(buf.data_ptr() + 1), stride))      # odd base
    refused(lib.kosk_tape_expand_device(ctx.handle, 2, C.c_char_p(blob), 32, C.c_void_p(buf.data_ptr()), stride + 4))      # stride not a multiple of 8
    refused(lib.kosk_tape_expand_device(ctx.handle, 2, C.c_char_p(blob), 32, C.c_void_p(buf.data_ptr()), stride - 8))      # stride below one tape
    refused(lib.kosk_tape_expand_device(ctx.handle, 2, C.c_char_p(blob), 16, C.c_void_p(buf.data_ptr()), stride))
    refused(lib.kosk_tape_expand_device(ctx.handle, 0, C.c_char_p(blob), 32, C.c_void_p(buf.data_ptr()), stride))
    refused(lib.kosk_tape_expand_device(ctx.handle, mb + 1, C.c_char_p(blob), 32, C.c_void_p(buf.data_ptr()), stride))
    refused(lib.kosk_tape_expand_device(ctx.handle, 2, None, 32, C.c_void_p(buf.data_ptr()), stride))
    host_tapes = C.create_string_buffer(2 * stride)
    refused(lib.kosk_tape_expand_device(ctx.handle, 2, C.c_char_p(blob), 32, host_tapes, stride))                           # tapes in host memory
    assert bytes(buf.cpu().numpy()) == bytes([SENTINEL]) * (mb * stride + 64)  # nothing was started
    assert ctx.path_counts()["tape_expand"] == before
    for mode in (2, -1, 7):
        refused(lib.kosk_set_entropy(ctx.handle, mode))
    assert lib.kosk_set_entropy(None, 1) == -1
    # the handle works, and is still in the default mode
    tapes = [hashlib_tape(k, s) for s in seeds]
    want = ctx.verifiable_keygen(tapes)
    assert ctx.verifiable_keygen(seeds=seeds) == want
    assert want[2][0] == oracle.verifiable_keygen(k, tapes[0])[2]
    assert ctx.verify(want[2], want[0]) == [True] * mb
    calls = []
    ctx.set_randombytes(lambda nb: calls.append(nb) or bytes(nb))
    ctx.verifiable_keygen(None, n=1)
    assert calls[0] == 64 and len(calls) == oracle.params(k).tape_calls
    ctx.close()


def test_graph_replay_with_seeded_calls(torch_cuda, gpu_child):
    """tests/gpu_child_seeded.py: seeded_graph_replay -- KOSK_GRAPHS=1, seeded calls, device tapes and host tapes alternating on one
    handle: the same bytes as the plain-launch path."""
    out = gpu_child("from tests.gpu_child_seeded import seeded_graph_replay; seeded_graph_replay()")
    assert "seeded_graph_replay ok 3" in out
