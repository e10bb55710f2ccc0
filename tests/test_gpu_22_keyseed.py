"""GPU tests of the proof randomness derived from the key (format kosk-keyseed-v1; csrc/kosk_fs_kernels.hip: k_keyseed;
kosk_keyseed_device, kosk_stage_prover_keys_derived, kosk_prove_keys_derived_batch).  References: the hashlib model tests/keyseed_model.py
for the seeds, the seeded calls on the model's seeds for whole proofs (which the suite pins to the oracle), and the CPU oracle's own prover
(plain for an unbound case, tests/bound_oracle.py for a bound one).  Every comparison is exact.  max_batch <= 3."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import keyproof_cases as kc
from tests import keyseed_model as km

pytestmark = pytest.mark.gpu

KS = km.KS


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


def _ctx_of(i):
    return bytes((7 * i + j) & 0xFF for j in range(32))


def _salt_of(i):
    return bytes((0xC3 ^ (11 * i + 5 * j)) & 0xFF for j in range(32))


def _seeds(k, sks, ctxs=None, salts=None):
    return [km.seed(k, sk, None if ctxs is None else ctxs[b], None if salts is None else salts[b]) for b, sk in enumerate(sks)]


def _same(got, want, what):
    assert len(got) == len(want)
    for b, (g, w) in enumerate(zip(got, want)):
        assert g == w, (what, b, _first_diff(g, w))


# ---- k_keyseed
@pytest.mark.parametrize("k", KS)
def test_keyseed_device_against_the_model(k, torch):
    """message lengths 1720 / 2488 / 3256 (last blocks of 88 / 40 / 128 bytes: at K = 4 both pad bytes share the last rate lane); the
    four flag combinations; n = 1, 3 and 65 (more than max_batch, more than a wave's worth of blocks); sk, contexts and salts each from
    host and from device memory; strides 32 and 40; the guard bands in front of and behind n x 32 bytes stay as they were"""
    api = _api()
    ctx = api.Kosk(kyber_k=k, max_batch=2)
    rng = np.random.default_rng(2200 + k)
    skb = ctx.sk_bytes
    fixed = km.fixture_keys(k)
    launches = 0
    for n in (1, 3, 65):
        sks = rng.integers(0, 256, size=(n, skb), dtype=np.uint8)
        for b in range(min(n, len(fixed))):
            sks[b] = np.frombuffer(fixed[b], np.uint8)
        d_sk = _dev(torch, sks)
        for flags in range(4):
            for sk_dev, cx_dev, sa_dev, cs, ss in ((False, False, False, 32, 40), (True, True, True, 40, 32), (False, True, False, 40, 40), (True, False, True, 32, 32)):
                cx = rng.integers(0, 256, size=(n, cs), dtype=np.uint8)
                sa = rng.integers(0, 256, size=(n, ss), dtype=np.uint8)
                d_cx, d_sa = _dev(torch, cx), _dev(torch, sa)
                want = [km.seed(k, sks[b].tobytes(), cx[b, :32].tobytes() if flags & 1 else None, sa[b, :32].tobytes() if flags & 2 else None)
                        for b in range(n)]
                d_out = torch.full(((n + 2) * 32,), 0xA5, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                ctx.keyseed_device(n, d_sk.data_ptr() if sk_dev else sks.tobytes(), d_out.data_ptr() + 32,
                                   contexts=None if not flags & 1 else d_cx.data_ptr() if cx_dev else cx.tobytes(), context_stride=cs,
                                   salts=None if not flags & 2 else d_sa.data_ptr() if sa_dev else sa.tobytes(), salt_stride=ss)
                launches += 1
                out = d_out.cpu().numpy()
                for b in range(n):
                    assert out[32 * (b + 1):32 * (b + 2)].tobytes() == want[b], (k, n, flags, sk_dev, cx_dev, sa_dev, cs, ss, b)
                assert (out[:32] == 0xA5).all() and (out[32 * (n + 1):] == 0xA5).all(), (k, n, flags, "guard bands")
    # device memory at a base that is no multiple of 8 (staged), next to the same records read in place
    odd = torch.zeros((3 * skb + 8,), dtype=torch.uint8, device="cuda")
    odd[4:4 + 3 * skb] = d_sk[:3].reshape(-1)
    d_out = torch.zeros((96,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.keyseed_device(3, odd.data_ptr() + 4, d_out.data_ptr())
    launches += 1
    assert d_out.cpu().numpy().tobytes() == b"".join(km.seed(k, sks[b].tobytes()) for b in range(3))
    # the pinned vectors, through the device
    vec = km.fixture()["k"]["k%d" % k]["vectors"]
    d_out = torch.zeros((32,), dtype=torch.uint8, device="cuda")
    for v in vec:
        ctx.keyseed_device(1, fixed[v["key"]], d_out.data_ptr(), contexts=km.PIN_CONTEXT if v["flags"] & 1 else None,
                           salts=km.PIN_SALT if v["flags"] & 2 else None)
        launches += 1
        assert d_out.cpu().numpy().tobytes().hex() == v["seed"], (k, v["key"], v["flags"])
    assert ctx.path_count(api.Kosk.PATH_KEYSEED) == launches
    # refused: a misaligned d_seeds, d_seeds in host memory, strides below 32, n = 0, a NULL sk -- with a text, and nothing is launched
    host_out = np.zeros(64, np.uint8)
    sk1 = fixed[0]
    for call in (lambda: ctx.keyseed_device(1, sk1, d_out.data_ptr() + 4), lambda: ctx.keyseed_device(1, sk1, host_out.ctypes.data),
                 lambda: ctx.keyseed_device(1, sk1, d_out.data_ptr(), contexts=bytes(32), context_stride=31),
                 lambda: ctx.keyseed_device(1, sk1, d_out.data_ptr(), salts=bytes(32), salt_stride=31),
                 lambda: ctx.keyseed_device(0, sk1, d_out.data_ptr()), lambda: ctx.keyseed_device(1, None, d_out.data_ptr())):
        with pytest.raises(api.KoskError):
            call()
    assert not host_out.any() and ctx.path_count(api.Kosk.PATH_KEYSEED) == launches
    ctx.keyseed_device(1, sk1, d_out.data_ptr())
    assert d_out.cpu().numpy().tobytes() == km.seed(k, sk1)
    ctx.close()


# ---- whole proofs
@pytest.mark.parametrize("fs", [0, 1])
@pytest.mark.parametrize("k", KS)
def test_derived_proofs_equal_the_seeded_proofs_of_the_model_seeds(k, fs, oracle, torch):
    """armed and unarmed, with and without salts: prove_keys(derived) = prove_keys(seeds = model seeds), byte for byte; for the unbound
    K = 3 case also the CPU oracle's own prover on the hashlib tape of the model's seed"""
    api = _api()
    n = 3
    sks = [kc.honest(k, i)[1] for i in range(n)]
    pks = [kc.honest(k, i)[0] for i in range(n)]
    ctxs, salts = [_ctx_of(b) for b in range(n)], [_salt_of(b) for b in range(n)]
    ctx = api.Kosk(kyber_k=k, max_batch=n, fs_mode=fs)
    seen = set()
    for armed in (False, True):
        if armed:
            ctx.set_contexts(ctxs)
        for salted in (False, True):
            seeds = _seeds(k, sks, ctxs if armed else None, salts if salted else None)
            got, ok = ctx.prove_keys(sks, derived=True, salts=salts if salted else None)
            want, ok2 = ctx.prove_keys(sks, seeds=seeds)
            assert ok == ok2 == [True] * n
            _same(got, want, (k, fs, armed, salted))
            assert ctx.verify(got, pks) == [True] * n
            seen.update(got)
            if k == 3 and not armed and not salted:
                ref = kc.oracle_proof(k, sks[0], km.tape_from_seed(k, seeds[0]))
                assert got[0] == ref, ("oracle", fs, _first_diff(got[0], ref))
    assert len(seen) == 4 * n  # every flag combination gave other proofs
    ctx.close()


@pytest.mark.parametrize("fs", [0, 1])
def test_bound_derived_proof_equals_the_bound_oracle(fs, oracle, torch):
    """the key of oracle tape 0; the derived model of tests/bound_oracle.py run on that tape's key seed followed by the hashlib tape of the
    model's seed (the key generation reads the first 64 bytes only, the prover everything behind them)"""
    from tests import bound_oracle as bo
    api = _api()
    k = 2
    context = bo.PIN_CONTEXT
    tape0 = oracle.tape_bytes_for(k, 0)
    pk, sk, _ = bo.pinned(k)
    seed = km.seed(k, sk, context)
    wpk, wsk, wpi = bo.verifiable_keygen(k, tape0[:64] + km.tape_from_seed(k, seed)[64:], context=context)
    assert (wpk, wsk) == (pk, sk)
    ctx = api.Kosk(kyber_k=k, max_batch=2, fs_mode=fs)
    ctx.set_contexts([context])
    got, ok = ctx.prove_keys([sk], derived=True)
    assert ok == [True] and got[0] == wpi, (fs, _first_diff(got[0], wpi))
    assert ctx.verify(got, [pk]) == [True] and bo.verify(k, got[0], pk, context=context)
    ctx.close()


def test_determinism_and_separation(torch):
    api = _api()
    k = 3
    pk, sk = kc.honest(k, 0)[:2]
    c1, c2 = _ctx_of(1), _ctx_of(2)
    ctx = api.Kosk(kyber_k=k, max_batch=2)

    def prove(context, salt=None):
        if context is None:
            ctx.clear_contexts()
        else:
            ctx.set_contexts([context])
        got, ok = ctx.prove_keys([sk], derived=True, salts=None if salt is None else [salt])
        assert ok == [True]
        return got[0]

    def accepts(context, pi):
        if context is None:
            ctx.clear_contexts()
        else:
            ctx.set_contexts([context])
        return ctx.verify([pi], [pk])[0]
    p1, p1_again, p2, p0 = prove(c1), prove(c1), prove(c2), prove(None)
    assert p1 == p1_again and len({p0, p1, p2}) == 3
    assert accepts(c1, p1) and accepts(c2, p2) and accepts(None, p0)
    assert not accepts(c2, p1) and not accepts(c1, p2) and not accepts(None, p1) and not accepts(c1, p0)
    s1 = prove(c1, _salt_of(0))
    assert s1 != p1 and s1 == prove(c1, _salt_of(0)) and s1 != prove(c1, _salt_of(1))
    assert accepts(c1, s1) and not accepts(c2, s1)
    # a zero context on an armed handle is not the unarmed handle, and a zero salt is not no salt
    z = prove(bytes(32))
    assert z != p0 and prove(None, bytes(32)) != p0
    # salts=True: fresh draws, two calls differ and both verify
    ctx.set_contexts([c1])
    a, _ = ctx.prove_keys([sk], derived=True, salts=True)
    b, _ = ctx.prove_keys([sk], salts=True)
    assert a[0] != b[0] and a[0] != p1 and accepts(c1, a[0]) and accepts(c1, b[0])
    ctx.close()


@pytest.mark.parametrize("streams", [1, 2])
def test_positions_follow_chunks_and_sub_batches(streams, torch):
    """max_batch = 2, n = 5, distinct contexts and salts: proof b of the call is the single-proof call under context b with salt b, and
    the seeded proof of the model's seed b"""
    api = _api()
    k, n = 2, 5
    sks = [kc.honest(k, i % 4)[1] for i in range(n)]
    ctxs, salts = [_ctx_of(10 + b) for b in range(n)], [_salt_of(10 + b) for b in range(n)]
    ctx = api.Kosk(kyber_k=k, max_batch=2, streams=streams)
    assert ctx.streams == streams
    ctx.set_contexts(ctxs)
    got, ok = ctx.prove_keys(sks, derived=True, salts=salts)
    assert ok == [True] * n
    want, _ = ctx.prove_keys(sks, seeds=_seeds(k, sks, ctxs, salts))
    _same(got, want, ("chunked", streams))
    # the staged form of one max_batch: the sub-batches of streams = 2 pass their offsets on
    assert ctx.stage_prover_keys(sks[:2], derived=True, salts=salts[:2]) == [True, True]
    ctx.prove_resident(2)
    _same(ctx.fetch_proofs(2), want[:2], ("staged", streams))
    for b in range(n):
        ctx.set_contexts([ctxs[b]])
        one, ok1 = ctx.prove_keys([sks[b]], derived=True, salts=[salts[b]])
        assert ok1 == [True] and one[0] == got[b], (streams, b, _first_diff(one[0], got[b]))
    ctx.close()


def test_resident_flow(torch):
    """stage_prover_keys(derived) -> prove_resident -> fetch_proofs_dense / _compact / plain -> verify_resident_pk(NULL); salts from
    device memory at stride 40"""
    api = _api()
    k, n = 3, 3
    sks = [kc.honest(k, i)[1] for i in range(n)]
    salts = [_salt_of(20 + b) for b in range(n)]
    ctx = api.Kosk(kyber_k=k, max_batch=n)
    images, ok = ctx.prove_keys(sks, derived=True, salts=salts)
    assert ok == [True] * n
    d_sa = _dev(torch, np.frombuffer(b"".join(s + bytes(8) for s in salts), np.uint8).copy())
    d_sk = _dev(torch, np.frombuffer(b"".join(sks), np.uint8).copy())
    assert ctx.stage_prover_keys(d_sk.data_ptr(), n=n, derived=True, salts=d_sa.data_ptr(), salt_stride=40) == [True] * n
    ctx.prove_resident(n)
    dense = ctx.fetch_proofs_dense(n)
    for b in range(n):
        rc, rec = api.dense_pack(k, images[b])
        assert rc == 0 and dense[b] == rec, ("dense", b)
    for b, blob in enumerate(ctx.fetch_proofs_compact(n)):
        out = C.create_string_buffer(ctx.proof_bytes)
        assert api.lib.kosk_proof_decompress(k, blob, out) == 0 and out.raw == images[b], ("compact", b)
    _same(ctx.fetch_proofs(n), images, "plain")
    assert ctx.verify_resident_pk(n) == [True] * n
    cts, sss, done = ctx.kem_enc_verified(n, coins=[bytes([b + 1]) * 32 for b in range(n)])
    assert done == [True] * n and ctx.kem_dec(cts, sks) == sss
    ctx.close()


def test_mixed_batch(torch):
    """a mismatched s-hat / pk record between two good keys: ok = [1, 0, 1], a zero image in the middle, the neighbours are their
    single-key proofs; the resident form leaves a proof that does not verify at the rejected position"""
    api = _api()
    k, n = 3, 3
    sks = [kc.honest(k, 0)[1], kc.pk_swapped(k), kc.honest(k, 2)[1]]
    ctx = api.Kosk(kyber_k=k, max_batch=n)
    got, ok = ctx.prove_keys(sks, derived=True)
    assert ok == [True, False, True] and got[1] == bytes(ctx.proof_bytes)
    for b in (0, 2):
        one, ok1 = ctx.prove_keys([sks[b]], derived=True)
        assert ok1 == [True] and one[0] == got[b], b
        assert one[0] == ctx.prove_keys([sks[b]], seeds=[km.seed(k, sks[b])])[0][0]
    assert ctx.stage_prover_keys(sks, derived=True) == [True, False, True]
    ctx.prove_resident(n)
    assert ctx.verify_resident_pk(n) == [True, False, True]
    ctx.close()


def test_argument_errors_leave_the_handle_usable(torch):
    api = _api()
    k, n = 2, 2
    ctx = api.Kosk(kyber_k=k, max_batch=n)
    lib, h = api.lib, ctx.handle
    sks = [kc.honest(k, i)[1] for i in range(n)]
    want, _ = ctx.prove_keys(sks, seeds=_seeds(k, sks))
    skb, salts = b"".join(sks), bytes(64)
    ok = C.create_string_buffer(8)
    pi = C.create_string_buffer(ctx.proof_bytes * (n + 1))
    count = ctx.path_count(api.Kosk.PATH_KEYSEED)
    assert count == 0
    bad = [
        lambda: lib.kosk_stage_prover_keys_derived(h, n, None, None, 0, ok),
        lambda: lib.kosk_stage_prover_keys_derived(h, n, skb, None, 0, None),
        lambda: lib.kosk_stage_prover_keys_derived(h, 0, skb, None, 0, ok),
        lambda: lib.kosk_stage_prover_keys_derived(h, n + 1, skb, None, 0, ok),
        lambda: lib.kosk_stage_prover_keys_derived(h, n, skb, salts, 31, ok),
        lambda: lib.kosk_prove_keys_derived_batch(h, n, None, None, 0, pi, ok),
        lambda: lib.kosk_prove_keys_derived_batch(h, n, skb, None, 0, None, ok),
        lambda: lib.kosk_prove_keys_derived_batch(h, n, skb, None, 0, pi, None),
        lambda: lib.kosk_prove_keys_derived_batch(h, 0, skb, None, 0, pi, ok),
        lambda: lib.kosk_prove_keys_derived_batch(h, n, skb, salts, 31, pi, ok),
    ]
    for i, call in enumerate(bad):
        assert call() == -1, i
        assert len(lib.kosk_last_error(h)) > 10, i
        if i % 5 == 4:
            assert ctx.prove_keys(sks, derived=True)[0] == want, i
            count += 1  # one chunk, one launch
    assert ctx.path_count(api.Kosk.PATH_KEYSEED) == count
    # more proofs than armed contexts: refused whole, the handle stays armed and usable
    ctx.set_contexts([_ctx_of(0)])
    for call in (lambda: ctx.prove_keys(sks, derived=True), lambda: ctx.stage_prover_keys(sks, derived=True)):
        with pytest.raises(api.KoskError, match="armed with fewer contexts"):
            call()
    assert ctx.path_count(api.Kosk.PATH_KEYSEED) == count
    one, ok1 = ctx.prove_keys(sks[:1], derived=True)
    assert ok1 == [True] and one == ctx.prove_keys(sks[:1], seeds=[km.seed(k, sks[0], _ctx_of(0))])[0]
    ctx.clear_contexts()
    assert ctx.prove_keys(sks, derived=True) == (want, [True] * n)
    # the counter counts launches: one per staged chunk (n = 3 on max_batch = 2: two), one per kernel-level call
    before = ctx.path_count(api.Kosk.PATH_KEYSEED)
    ctx.prove_keys(sks + sks[:1], derived=True)
    assert ctx.path_count(api.Kosk.PATH_KEYSEED) == before + 2
    with pytest.raises(api.KoskError):
        ctx.prove_keys(sks, derived=True, seeds=_seeds(k, sks))
    with pytest.raises(api.KoskError):
        ctx.prove_keys(sks, derived=True, salts=[bytes(32)])
    ctx.close()


def test_cohort_members_derive_unmerged(torch, gpu_child):
    """tests/gpu_child_keyseed.py: cohort_members_derive"""
    out = gpu_child("from tests.gpu_child_keyseed import cohort_members_derive; cohort_members_derive()")
    assert "cohort_members_derive ok 2" in out


@pytest.mark.parametrize("k", KS)
def test_reprove_derived_example(k, torch):
    """examples/reprove_derived.cpp on the C ABI: one key, two nonces, no entropy source and no stored seed"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "reprove_derived")
    if not os.path.exists(exe):
        pytest.fail("examples/reprove_derived missing: run __graft_entry__.build()")
    r = subprocess.run([exe, str(k)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 7 and all(ln.endswith("= 1") for ln in lines), r.stdout
    assert lines[-1] == "[result] reprove_derived success = 1"
