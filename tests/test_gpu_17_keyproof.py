"""GPU tests of the proofs for existing Kyber keys (include/kosk_mi355x.h: kosk_witness_from_sk, kosk_stage_prover_keys[_seeded],
kosk_prove_keys[_seeded]_batch).  References: the proofs of verifiable_keygen on the same tapes (which the suite pins to the oracle),
api.host_keygen's s and e, the pure-Python model of tests/keyproof_cases.py, and the CPU oracle's own prover for keys this library
never made.  Every comparison is exact.  One handle at a time, max_batch <= 8."""
import ctypes as C

import numpy as np
import pytest

from tests import keyproof_cases as kc

pytestmark = pytest.mark.gpu

KS = kc.KS


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return torch


def _api():
    from mpcith_kyber_kosk_amd import api
    return api


def _first_diff(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), None)


@pytest.mark.parametrize("fs", [0, 1])
@pytest.mark.parametrize("k", KS)
def test_proofs_equal_the_verifiable_keygen_of_the_same_tapes(k, fs, oracle, torch_cuda):
    """the normative rule: on the sk that verifiable_keygen(tape) returned, prove_keys(sk, tape) is that call's proof byte for byte --
    and the first 64 bytes of the tape (the key seed) are not read"""
    api = _api()
    n = 3
    tapes = [oracle.tape_bytes_for(k, i) for i in range(n)]
    ctx = api.Kosk(kyber_k=k, max_batch=n, fs_mode=fs)
    pks, sks, pis = ctx.verifiable_keygen(tapes)
    got, ok = ctx.prove_keys(sks, tapes)
    assert ok == [True] * n
    for b in range(n):
        assert got[b] == pis[b], (k, fs, b, _first_diff(got[b], pis[b]))
    blind = [b"\xff" * 64 + t[64:] for t in tapes]
    got2, ok2 = ctx.prove_keys(sks, blind)
    assert ok2 == [True] * n and got2 == pis
    assert ctx.verify(got, pks) == [True] * n
    ctx.close()


@pytest.mark.parametrize("k", KS)
def test_witness_equals_the_key_generation(k, torch_cuda):
    """witness_from_sk = host_keygen's s, e at n = 8 and n = 1, sk in host and in device memory; the n = 1 calls come after the larger
    one on the same handle (a stale workspace would show), and a rejected key after accepted ones is all zero"""
    api = _api()
    torch = torch_cuda
    ctx = api.Kosk(kyber_k=k, max_batch=8)
    keys = [kc.honest(k, i) for i in range(8)]
    want = np.array([kc.se_rows(s, e) for _, _, s, e in keys], np.int16).reshape(8, 2 * k, 256)
    se, ok = ctx.witness_from_sk([key[1] for key in keys])
    assert ok == [True] * 8 and np.array_equal(se, want)
    dev = torch.frombuffer(bytearray(b"".join(key[1] for key in keys)), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    se, ok = ctx.witness_from_sk(dev.data_ptr(), n=8)
    assert ok == [True] * 8 and np.array_equal(se, want)
    for i in (5, 2):  # n = 1 after n = 8: another key than the one at position 0 of the last call
        se, ok = ctx.witness_from_sk([keys[i][1]])
        assert ok == [True] and np.array_equal(se[0], want[i])
        se, ok = ctx.witness_from_sk(dev.data_ptr() + i * ctx.sk_bytes, n=1)
        assert ok == [True] and np.array_equal(se[0], want[i])
    se, ok = ctx.witness_from_sk([kc.pk_swapped(k), keys[3][1]])
    assert ok == [False, True] and not se[0].any() and np.array_equal(se[1], want[3])
    folded, changed = kc.noncanonical_shat(k, keys[6][1])
    se, ok = ctx.witness_from_sk([folded])
    assert changed > 0 and ok == [True] and np.array_equal(se[0], want[6])
    ctx.close()


@pytest.mark.parametrize("k", KS)
def test_seeded_equals_the_tapes_of_the_seeds(k, torch_cuda):
    api = _api()
    from tests.gpu_child_seeded import seed_for
    n = 3
    ctx = api.Kosk(kyber_k=k, max_batch=n)
    sks = [kc.honest(k, i)[1] for i in range(n)]
    seeds = [seed_for(k, i, "keyproof") for i in range(n)]
    want, ok = ctx.prove_keys(sks, tapes=[api.tape_from_seed(k, s) for s in seeds])
    got, ok2 = ctx.prove_keys(sks, seeds=seeds)
    assert ok == ok2 == [True] * n and got == want
    assert ctx.stage_prover_keys(sks, seeds=seeds) == [True] * n
    ctx.prove_resident(n)
    assert ctx.fetch_proofs(n) == want
    ctx.close()


@pytest.mark.parametrize("k", KS)
def test_entropy_modes_without_tapes(k, torch_cuda):
    """tapes = None: tape mode draws the reference's sequence without the key generation's 64 bytes (M x 32, then nfresh x 302); seed
    mode one 32-byte draw per proof"""
    api = _api()
    import hashlib
    n = 2
    ctx = api.Kosk(kyber_k=k, max_batch=n)
    sks = [kc.honest(k, i)[1] for i in range(n)]
    T = ctx.tape_bytes
    stream = hashlib.shake_256(b"kosk-keyproof-v1:entropy:%d" % k).digest(n * (T - 64))
    state, sizes = [0], []

    def rb(nbytes):
        sizes.append(nbytes)
        state[0] += nbytes
        return stream[state[0] - nbytes:state[0]]
    ctx.set_randombytes(rb)
    got, ok = ctx.prove_keys(sks)
    assert ok == [True] * n and state[0] == n * (T - 64) and 64 not in sizes and set(sizes) == {32, 302}
    tapes = [bytes(64) + stream[b * (T - 64):(b + 1) * (T - 64)] for b in range(n)]
    assert got == ctx.prove_keys(sks, tapes)[0]
    ctx.set_entropy(api.ENTROPY_SEED)
    state[0], sizes[:] = 0, []
    got, ok = ctx.prove_keys(sks)
    assert ok == [True] * n and sizes == [32] * n
    assert got == ctx.prove_keys(sks, seeds=[stream[32 * b:32 * b + 32] for b in range(n)])[0]
    ctx.close()


@pytest.mark.parametrize("k", KS)
def test_foreign_keys(k, oracle, torch_cuda):
    """key pairs of the reference's crypto_kem_keypair_derand: the proofs verify under Kosk.verify and under the oracle, and are the
    oracle's own proofs for those instances"""
    api = _api()
    keys = kc.foreign(k)
    tapes = [oracle.tape_bytes_for(k, 40 + i) for i in range(len(keys))]
    ctx = api.Kosk(kyber_k=k, max_batch=2)
    got, ok = ctx.prove_keys([sk for _, sk in keys], tapes)
    assert ok == [True, True]
    assert ctx.verify(got, [pk for pk, _ in keys]) == [True, True]
    for b, (pk, sk) in enumerate(keys):
        assert oracle.kosk_verify(k, got[b], pk)[0], oracle.kosk_verify(k, got[b], pk)[1]
        want = kc.oracle_proof(k, sk, tapes[b])
        assert got[b] == want, (k, b, _first_diff(got[b], want))
    ctx.close()


@pytest.mark.parametrize("k", KS)
def test_range_edges_in_mixed_batches(k, oracle, torch_cuda):
    """the crafted keys of the CPU test (72 edge cases, the two extreme keys, a pk swap and an honest key) in batches of 8 that mix
    accepted and rejected positions: ok as expected, rejected images all zero, every accepted position byte-equal to the same key
    proven alone with the same tape, and verified"""
    api = _api()
    cases = [(name, sk, acc) for name, sk, acc in kc.range_edges(k)]
    ext = kc.extreme_keys(k)
    cases += [(ext[0][0], ext[0][1], True), ("pk swap", kc.pk_swapped(k), False), (ext[1][0], ext[1][1], True), ("honest", kc.honest(k, 1)[1], True)]
    cases += cases[2:6]  # 80 = 10 batches of 8
    assert len(cases) == 80
    tapes = [oracle.tape_bytes_for(k, 60 + b) for b in range(8)]
    ctx = api.Kosk(kyber_k=k, max_batch=8)
    zero = bytes(ctx.proof_bytes)
    for first in range(0, 80, 8):
        batch = cases[first:first + 8]
        want_ok = [c[2] for c in batch]
        assert True in want_ok and False in want_ok
        got, ok = ctx.prove_keys([c[1] for c in batch], tapes)
        assert ok == want_ok, (k, [c[0] for c in batch])
        acc = [b for b in range(8) if want_ok[b]]
        for b in range(8):
            if not want_ok[b]:
                assert got[b] == zero, (k, batch[b][0])
        pks = [batch[b][1][384 * k:768 * k + 32] for b in acc]
        assert ctx.verify([got[b] for b in acc], pks) == [True] * len(acc), (k, [batch[b][0] for b in acc])
        for b in acc:
            alone, ok1 = ctx.prove_keys([batch[b][1]], [tapes[b]])
            assert ok1 == [True] and alone[0] == got[b], (k, batch[b][0])
    ctx.close()


def test_chunking(oracle, torch_cuda):
    """max_batch = 4, n = 9 (a rejected key inside the second chunk): the bytes of the one-at-a-time calls"""
    api = _api()
    k, n = 3, 9
    ctx = api.Kosk(kyber_k=k, max_batch=4)
    sks = [kc.honest(k, i % 8)[1] for i in range(n)]
    sks[5] = kc.pk_swapped(k)
    tapes = [oracle.tape_bytes_for(k, 80 + i) for i in range(n)]
    got, ok = ctx.prove_keys(sks, tapes)
    assert ok == [b != 5 for b in range(n)] and got[5] == bytes(ctx.proof_bytes)
    for b in range(n):
        one, ok1 = ctx.prove_keys([sks[b]], [tapes[b]])
        assert ok1 == [b != 5] and one[0] == got[b], b
    ctx.close()


def test_resident_flow(oracle, torch_cuda):
    """stage_prover_keys -> prove_resident -> verify_resident_pk(pk = NULL) -> kem_enc_verified -> kem_dec with the same secret keys;
    the compact fetch decompresses to the images"""
    api = _api()
    k, n = 3, 4
    ctx = api.Kosk(kyber_k=k, max_batch=n)
    keys = [kc.honest(k, 0), kc.honest(k, 1)] + [(pk, sk, None, None) for pk, sk in kc.foreign(k)]
    sks = [key[1] for key in keys]
    tapes = [oracle.tape_bytes_for(k, 90 + i) for i in range(n)]
    assert ctx.stage_prover_keys(sks, tapes) == [True] * n
    ctx.prove_resident(n)
    images = ctx.fetch_proofs(n)
    assert images == ctx.prove_keys(sks, tapes)[0]
    assert ctx.stage_prover_keys(sks, tapes) == [True] * n
    ctx.prove_resident(n)
    cb = api.lib.kosk_compact_proof_bytes(k)
    for b, blob in enumerate(ctx.fetch_proofs_compact(n)):
        out = C.create_string_buffer(ctx.proof_bytes)
        assert len(blob) == cb and api.lib.kosk_proof_decompress(k, blob, out) == 0 and out.raw == images[b], b
    assert ctx.verify_resident_pk(n) == [True] * n
    cts, sss, done = ctx.kem_enc_verified(n, coins=[bytes([b + 1]) * 32 for b in range(n)])
    assert done == [True] * n
    assert ctx.kem_dec(cts, sks) == sss and len(set(sss)) == n
    want_ct, want_ss = ctx.kem_enc([key[0] for key in keys], [bytes([b + 1]) * 32 for b in range(n)])
    assert (cts, sss) == (want_ct, want_ss)
    ctx.close()


def test_resident_proof_of_a_rejected_key_does_not_verify(oracle, torch_cuda):
    """the resident form leaves, at a position with ok = 0, a proof made from the zero witness: it does not verify, the others do"""
    api = _api()
    k, n = 3, 4
    ctx = api.Kosk(kyber_k=k, max_batch=n)
    sks = [kc.honest(k, i)[1] for i in range(n)]
    sks[2] = kc.pk_swapped(k)
    tapes = [oracle.tape_bytes_for(k, 110 + i) for i in range(n)]
    assert ctx.stage_prover_keys(sks, tapes) == [True, True, False, True]
    ctx.prove_resident(n)
    assert ctx.verify_resident_pk(n) == [True, True, False, True]
    cts, sss, done = ctx.kem_enc_verified(n, coins=[bytes([b + 1]) * 32 for b in range(n)])
    assert done == [True, True, False, True] and cts[2] == bytes(len(cts[2])) and sss[2] == bytes(32)
    ctx.close()


def test_argument_errors_leave_the_handle_usable(oracle, torch_cuda):
    api = _api()
    k, n = 2, 2
    ctx = api.Kosk(kyber_k=k, max_batch=n)
    lib, h = api.lib, ctx.handle
    sks = [kc.honest(k, i)[1] for i in range(n)]
    tapes = [oracle.tape_bytes_for(k, 100 + i) for i in range(n)]
    want, _ = ctx.prove_keys(sks, tapes)
    skb, tpb = b"".join(sks), b"".join(tapes)
    T, S = ctx.tape_bytes, 32
    ok = C.create_string_buffer(8)
    pi = C.create_string_buffer(ctx.proof_bytes * n)
    se = np.zeros((n, 2 * k, 256), np.int16)
    seeds = bytes(64)
    bad = [
        lambda: lib.kosk_witness_from_sk(h, 0, skb, se.ctypes.data, ok),
        lambda: lib.kosk_witness_from_sk(h, n + 1, skb, se.ctypes.data, ok),
        lambda: lib.kosk_witness_from_sk(h, n, None, se.ctypes.data, ok),
        lambda: lib.kosk_witness_from_sk(h, n, skb, se.ctypes.data, None),
        lambda: lib.kosk_stage_prover_keys(h, 0, skb, tpb, T, ok),
        lambda: lib.kosk_stage_prover_keys(h, n + 1, skb, tpb, T, ok),
        lambda: lib.kosk_stage_prover_keys(h, n, None, tpb, T, ok),
        lambda: lib.kosk_stage_prover_keys(h, n, skb, tpb, T, None),
        lambda: lib.kosk_stage_prover_keys(h, n, skb, tpb, T - 1, ok),
        lambda: lib.kosk_stage_prover_keys_seeded(h, 0, skb, seeds, S, ok),
        lambda: lib.kosk_stage_prover_keys_seeded(h, n + 1, skb, seeds, S, ok),
        lambda: lib.kosk_stage_prover_keys_seeded(h, n, None, seeds, S, ok),
        lambda: lib.kosk_stage_prover_keys_seeded(h, n, skb, seeds, S - 1, ok),
        lambda: lib.kosk_prove_keys_batch(h, 0, skb, tpb, T, pi, ok),
        lambda: lib.kosk_prove_keys_batch(h, n, None, tpb, T, pi, ok),
        lambda: lib.kosk_prove_keys_batch(h, n, skb, tpb, T, None, ok),
        lambda: lib.kosk_prove_keys_batch(h, n, skb, tpb, T, pi, None),
        lambda: lib.kosk_prove_keys_batch(h, n, skb, tpb, T - 1, pi, ok),
        lambda: lib.kosk_prove_keys_seeded_batch(h, n, skb, seeds, S - 1, pi, ok),
        lambda: lib.kosk_prove_keys_seeded_batch(h, n, skb, seeds, S, None, ok),
    ]
    for i, call in enumerate(bad):
        assert call() == -1, i
        assert len(lib.kosk_last_error(h)) > 10, i
        if i % 5 == 4:
            assert ctx.prove_keys(sks, tapes)[0] == want, i
    assert ctx.prove_keys(sks, tapes) == (want, [True] * n)
    ctx.close()
