"""Every position of a batch against the oracle's pinned digests (tests/oracle_pins.py), over the batch sizes where the persistent
kernels deal their work units differently, over context shapes and both Fiat-Shamir modes; and the verifier's bits and fail masks
at every position of batches that mix honest proofs with one-change corruptions, against the oracle's live verdicts.

A kernel bug that depends on a proof's content and not on its position corrupts the prover and the verifier alike (they share the
key generation, the table product, the commitment hashes and the alpha powers): verify still says True and a second GPU handle
still agrees.  Only the oracle catches it, so every tape here lands at several positions and every position is compared."""
import concurrent.futures as cf
import functools
import os

import numpy as np
import pytest

from tests import oracle_lib as oracle
from tests import oracle_pins

pytestmark = pytest.mark.gpu

Q = 3329
WINDOW = {2: (0, 160), 3: (0, 128), 4: (2000, 160)}    # (first tape, width) of the sliding windows of the size sweeps
SHAPE_TAPES = (0, 512)                                  # K = 3 tapes of the context-shape cases
PLANS = ((2, 46, 0), (3, 64, 100))                      # (K, n, first tape) of the verifier plans


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return torch


def pinned_tapes():
    """{K: tape indices} this module reads (tests/test_oracle_pins.py checks that the fixture covers them)"""
    out = {k: set(range(s, s + w)) for k, (s, w) in WINDOW.items()}
    out[3] |= set(range(*SHAPE_TAPES))
    for k, n, s in PLANS:
        out[k] |= set(range(s, s + n))
    return out


@functools.lru_cache(maxsize=None)
def _tape(k, idx):
    return oracle.tape_bytes_for(k, idx)


# ---- batch sizes at the work-distribution boundaries of the persistent kernels ----------------------------------------------------
# k_lincomb_stream (launch_lincomb_stream, csrc/kosk_kernels.hip): 2 * ceil(NPTS / 128) = 28 (group, point block) units per proof,
# dealt over min(28 n, 2 CUs) workgroups.  A workgroup gets a second unit (and first reloads its group: g != g_cur) once 28 n > 2 CUs,
# a third once 28 n > 4 CUs: n = 19 and 37 on 256 CUs.
def lincomb_stream_edges(ncu):
    return [2 * ncu // 28 + 1, 4 * ncu // 28 + 1]


# k_table_gemm_p (launch_table_gemm, 7 k-steps): rows = (rows per proof) x n, nblk = ceil(rows / 48) row blocks, nchunks = M / 16
# table chunks, total = nblk x nchunks (row block, chunk) units over nwg = min(total / 8, CUs) workgroups; workgroup w takes units
# [w total / nwg, (w + 1) total / nwg).  Two things change with n: nwg stops growing with the product (total / 8 reaches the CU count)
# and the whole row blocks a workgroup's unit range covers (at most ceil(total / nwg) / nchunks of them) go 0 -> 1 -> 2.  The
# prover's expansion has nfresh rows per proof and M = 1344 (84 chunks); the verifier's reconstruction 2 x 70 rows and M = 256.
def _table_gemm_state(rows, nchunks, ncu):
    nblk = -(-rows // 48)
    total = nblk * nchunks
    nwg = max(1, min(total // 8, ncu))
    return nwg == ncu, -(-total // nwg) // nchunks


def table_gemm_edges(k, ncu, nmax):
    p = oracle.params(k)
    nfresh = p.tape_calls - 1 - p.M
    out = set()
    for rows, nchunks in ((nfresh, 84), (140, 16)):
        out |= {n for n in range(2, nmax + 1) if _table_gemm_state(rows * n, nchunks, ncu) != _table_gemm_state(rows * (n - 1), nchunks, ncu)}
    return sorted(out)


def _ncu(torch):
    return torch.cuda.get_device_properties(0).multi_processor_count


def _around(edges, nmax):
    return {m for e in edges for m in (e - 1, e, e + 1) if 1 <= m <= nmax}


def _sweep(ctx, k, ns, resident_odd=True):
    """one batch per n from a window that slides with n (each tape lands at several positions); every pk / sk / proof against the pins
    and every verify bit; proofs are hashed batch by batch and dropped"""
    first, width = WINDOW[k]
    fails = []
    for i, n in enumerate(ns):
        s = first + (n * 29) % (width - n + 1)
        idx = list(range(s, s + n))
        tapes = [_tape(k, j) for j in idx]
        if resident_odd and i % 2:
            ctx.verifiable_keygen_resident(tapes)
            pks, sks = ctx.keys(n)
            pis = ctx.fetch_proofs(n)
            ok = ctx.verify_resident_pk(n)
        else:
            pks, sks, pis = ctx.verifiable_keygen(tapes)
            ok = ctx.verify(pis, pks)
        mism = oracle_pins.check(k, idx, pks, sks, pis)
        rejected = [b for b, x in enumerate(ok) if not x]
        if mism or rejected or len(ok) != n:
            fails.append({"n": n, "first tape": s, "differ from the oracle (position, tape, fields)": mism, "rejected positions": rejected})
        del pks, sks, pis
    assert not fails, fails


def test_size_sweep_kyber768_every_n_up_to_64(torch_cuda):
    """K = 3, one context of max_batch 64, every n = 1..64 (host-buffer and resident calls in turn)"""
    from mpcith_kyber_kosk_amd import api
    ctx = api.Kosk(kyber_k=3, max_batch=64)
    _sweep(ctx, 3, list(range(1, 65)))
    ctx.close()


@pytest.mark.parametrize("k", [2, 4])
def test_size_sweep_at_work_distribution_edges(k, torch_cuda):
    """K = 2 and 4: small n, the k_lincomb_stream edges (18-20 and 36-38 on 256 CUs) and the k_table_gemm_p edges of this device,
    each with its neighbours"""
    from mpcith_kyber_kosk_amd import api
    nmax = WINDOW[k][1] * 3 // 4
    ncu = _ncu(torch_cuda)
    ns = set(range(1, 10)) | set(range(15, 21)) | set(range(31, 34)) | set(range(36, 39)) | set(range(45, 48))
    ns |= _around(lincomb_stream_edges(ncu), nmax) | _around(table_gemm_edges(k, ncu, nmax), nmax)
    ns = sorted(n for n in ns if n <= nmax)
    ctx = api.Kosk(kyber_k=k, max_batch=max(ns))
    _sweep(ctx, k, ns)
    ctx.close()


@pytest.mark.parametrize("fs", [0, 1])
@pytest.mark.parametrize("mb", [1, 47, 139])
def test_context_shapes(mb, fs, torch_cuda):
    """K = 3 contexts of max_batch 1, 47 and 139, at n = max_batch and max_batch - 1, with the Fiat-Shamir hashes on the host
    and on the device"""
    from mpcith_kyber_kosk_amd import api
    k = 3
    ctx = api.Kosk(kyber_k=k, max_batch=mb, fs_mode=fs)
    fails = []
    for n, s in ((mb, mb), (mb - 1, mb + 1)):
        if n < 1:
            continue
        idx = list(range(s, s + n))
        assert idx[-1] < SHAPE_TAPES[1]
        pks, sks, pis = ctx.verifiable_keygen([_tape(k, j) for j in idx])
        ok = ctx.verify(pis, pks)
        mism = oracle_pins.check(k, idx, pks, sks, pis)
        if mism or ok != [True] * n:
            fails.append((n, s, mism, [b for b, x in enumerate(ok) if not x]))
    assert (ctx.path_counts()["fs_device"] > 0) == bool(fs)
    ctx.close()
    assert not fails, fails


# ---- verifier positions -----------------------------------------------------------------------------------------------------------
def _t_noncanonical(k, pk, rng):
    """pk with one t coefficient c < 4096 - q re-encoded as the 12-bit value c + q (the same residue)"""
    b = bytearray(pk)
    ncoef = 256 * k
    start = int(rng.integers(ncoef))
    for m in range(ncoef):
        i = (start + m) % ncoef
        g = 3 * (i // 2)
        x = b[g] | (b[g + 1] << 8) | (b[g + 2] << 16)
        c = (x >> (12 * (i & 1))) & 0xFFF
        if c < 4096 - Q:
            x = (x & ~(0xFFF << (12 * (i & 1)))) | ((c + Q) << (12 * (i & 1)))
            b[g:g + 3] = x.to_bytes(3, "little")
            return bytes(b), i
    raise AssertionError("no t coefficient below 4096 - q")


def corruption_plan(k, pis, pks, first_field, seed):
    """[(proof, pk, label)] for every position: about half honest, the rest one change each -- a neighbour's pk, a flipped rho byte,
    a non-canonical t coefficient, then the proof fields in turn from first_field (a u16 element moved to another canonical residue,
    a byte of a digest field flipped)"""
    rng = np.random.default_rng(seed)
    p = oracle.params(k)
    n = len(pis)
    bad = sorted(int(x) for x in rng.choice(n, n - n // 2, replace=False))
    plan = [(pis[b], pks[b], "honest") for b in range(n)]
    for j, b in enumerate(bad):
        pi, pk = pis[b], pks[b]
        if j == 0:
            plan[b] = (pi, pks[(b + 1) % n], "pk of tape position %d" % ((b + 1) % n))
        elif j == 1:
            x = bytearray(pk); o = len(pk) - 32 + int(rng.integers(32)); x[o] ^= 1 << int(rng.integers(8))
            plan[b] = (pi, bytes(x), "rho byte %d" % o)
        elif j == 2:
            x, i = _t_noncanonical(k, pk, rng)
            plan[b] = (pi, x, "t coefficient %d + q" % i)
        else:
            f = (first_field + j - 3) % 24
            x = bytearray(pi)
            if f in (4, 23):   # tcomm, comm: 32-byte digests
                o = p.off[f] + int(rng.integers(p.size[f])); x[o] ^= int(rng.integers(1, 256))
                what = "field %d byte %d" % (f, o - p.off[f])
            else:
                e = int(rng.integers(p.size[f] // 2)); o = p.off[f] + 2 * e
                v = x[o] | (x[o + 1] << 8)
                nv = (v + int(rng.integers(1, Q))) % Q
                x[o:o + 2] = nv.to_bytes(2, "little")
                what = "field %d element %d: %d -> %d" % (f, e, v, nv)
            plan[b] = (bytes(x), pk, what)
    return plan


def _oracle_bits(k, plan):
    oracle.kosk_verify(k, plan[0][0], plan[0][1])  # tables built by one thread
    with cf.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        return list(ex.map(lambda e: oracle.kosk_verify(k, e[0], e[1]), plan))


@pytest.mark.parametrize("k,n,first", PLANS)
def test_verifier_positions_against_the_oracle(k, n, first, torch_cuda):
    """a seeded corruption plan at three rotations (every change visits three positions): at every position the GPU bit equals
    the oracle's, the fail mask is nonzero exactly when the bit is False, and a host-FS and a device-FS handle give equal masks"""
    from mpcith_kyber_kosk_amd import api
    hh = api.Kosk(kyber_k=k, max_batch=n, fs_mode=api.FS_HOST)
    hd = api.Kosk(kyber_k=k, max_batch=n, fs_mode=api.FS_DEVICE)
    idx = list(range(first, first + n))
    pks, sks, pis = hh.verifiable_keygen([_tape(k, j) for j in idx])
    oracle_pins.assert_batch(k, idx, pks, sks, pis)
    plan = corruption_plan(k, pis, pks, first_field=0 if n == 46 else 20, seed=1000 * k + n)
    exp = _oracle_bits(k, plan)
    changed = sum(x[2] != "honest" for x in plan)
    assert all(e[0] for e, x in zip(exp, plan) if x[2] == "honest") and changed >= n // 2
    # the reference accepts a change in an element it never reads (or one it only reduces), so not every change is a reject
    assert sum(not e[0] for e in exp) >= changed // 2
    fails = []
    for rot in (0, 17, n - 5):
        order = [(b + rot) % n for b in range(n)]   # position b holds plan entry order[b]
        rp = [plan[j][0] for j in order]
        rk = [plan[j][1] for j in order]
        gh = hh.verify(rp, rk); mh = hh.fail_masks(n)
        gd = hd.verify(rp, rk); md = hd.fail_masks(n)
        for b, j in enumerate(order):
            want = exp[j][0]
            if gh[b] != want or gd[b] != want or (mh[b] != 0) == want or mh[b] != md[b]:
                fails.append({"rotation": rot, "position": b, "change": plan[j][2], "oracle": exp[j], "host fs": (gh[b], hex(mh[b])),
                              "device fs": (gd[b], hex(md[b]))})
    assert not fails, fails
    rolled = pks[-1:] + pks[:-1]
    assert hh.verify(pis, rolled) == [False] * n and hd.verify(pis, rolled) == [False] * n
    hh.close()
    hd.close()
