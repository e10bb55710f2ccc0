"""GPU parity of the individual kernels (through the C-ABI, device pointers) vs hashlib / the oracle."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return t


@pytest.fixture(scope="module")
def ctx(torch):
    from mpcith_kyber_kosk_amd import api
    c = api.Kosk(kyber_k=3, max_batch=8)
    yield c
    c.close()


def _dev(torch, arr):
    return torch.from_numpy(np.ascontiguousarray(arr)).cuda()


@pytest.mark.parametrize("length", [0, 1, 31, 32, 33, 135, 136, 137, 271, 272, 320, 472, 1000])
def test_sha3_256_and_shake256_message_major(length, torch, ctx):
    n = 257  # ragged: not a multiple of the wave size
    rng = np.random.default_rng(length)
    stride = max(8, (length + 7) // 8 * 8)
    msgs = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
    d_in = _dev(torch, msgs)
    d_out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # torch fills / copies run on the null stream; the library streams are not ordered against it
    ctx.sha3_256_batch(d_in.data_ptr(), stride, length, d_out.data_ptr(), n)
    d_x = torch.zeros((n, 200), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # torch fills / copies run on the null stream; the library streams are not ordered against it
    ctx.shake256_batch(d_in.data_ptr(), stride, length, d_x.data_ptr(), 200, n)
    ctx.synchronize()
    out, xof = d_out.cpu().numpy(), d_x.cpu().numpy()
    for i in range(n):
        m = msgs[i, :length].tobytes()
        assert out[i].tobytes() == hashlib.sha3_256(m).digest()
        assert xof[i].tobytes() == hashlib.shake_256(m).digest(200)


@pytest.mark.parametrize("length", [0, 1, 3, 4, 5, 135, 136, 137, 271, 272, 320, 472, 1000])
def test_sha3_256_lane_pair_sponge(length, torch, ctx):
    """kosk_sha3_256_batch_pair: the lane-pair ("warp-cooperative") Keccak layout, 32 messages per wave, ragged counts (idle
    pairs in the last wave, a single message, one more than a wave) against hashlib."""
    rng = np.random.default_rng(1000 + length)
    stride = max(8, (length + 7) // 8 * 8)
    for n in (257, 1, 33):
        msgs = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
        d_in = _dev(torch, msgs)
        d_out = torch.zeros((n + 1, 32), dtype=torch.uint8, device="cuda")   # one guard row behind the last digest
        torch.cuda.synchronize()  # torch fills / copies run on the null stream; the library streams are not ordered against it
        ctx.sha3_256_batch_pair(d_in.data_ptr(), stride, length, d_out.data_ptr(), n)
        ctx.synchronize()
        out = d_out.cpu().numpy()
        for i in range(n):
            assert out[i].tobytes() == hashlib.sha3_256(msgs[i, :length].tobytes()).digest(), (n, i)
        assert not out[n].any()


@pytest.mark.parametrize("k", [2, 3, 4])
@pytest.mark.parametrize("with_prefix", [0, 1])
def test_commit_hash_column_layout(k, with_prefix, torch, oracle):
    """Both row layouts in every case (one pytest parameter more would rename the cases).  Stride 1600: 16-byte aligned rows that
    cover the last wave's 64 lanes, the LDS-DMA kernel.  Stride 1531 = the lane count, odd: rows that take neither 16-byte loads nor
    a read past lane n - 1, the plain kernel (24 waves: its pipelined variant, all six (PREFIX_WORDS, NROWS) instantiations)."""
    for stride in (1600, 1531):
        _commit_hash_column_layout(k, with_prefix, stride, torch, oracle)


def _commit_hash_column_layout(k, with_prefix, stride, torch, oracle):
    from mpcith_kyber_kosk_amd import api
    p = oracle.params(k)
    words = (p.view_msg_bytes - 32) // 2 if with_prefix else p.tcomm_msg_bytes // 2
    n = 1454 + 77  # ragged lane count
    rng = np.random.default_rng(100 * k + with_prefix)
    rows = rng.integers(0, 3329, size=(words, stride), dtype=np.uint16)
    prefix = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    c = api.Kosk(kyber_k=k, max_batch=1)
    d_rows, d_pre = _dev(torch, rows), _dev(torch, prefix)
    d_out = torch.zeros((n, 32), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()  # torch fills / copies run on the null stream; the library streams are not ordered against it
    c.commit_hash_lanes(d_rows.data_ptr(), stride, n, d_pre.data_ptr(), with_prefix, d_out.data_ptr())
    c.synchronize()
    out = d_out.cpu().numpy()
    for l in list(range(0, n, 97)) + [n - 1]:
        msg = (prefix[l].tobytes() if with_prefix else b"") + rows[:, l].astype("<u2").tobytes()
        assert out[l].tobytes() == hashlib.sha3_256(msg).digest(), (stride, l)
    # every lane
    cols = np.ascontiguousarray(rows[:, :n].T).astype("<u2")
    bad = [l for l in range(n) if out[l].tobytes() != hashlib.sha3_256((prefix[l].tobytes() if with_prefix else b"") + cols[l].tobytes()).digest()]
    assert not bad, ("lanes whose digest differs from hashlib", stride, len(bad), bad[:32])
    paths = c.path_counts()
    if stride % 8:
        assert paths["hash_plain"] == 1 and paths["hash_dma"] == 0, (stride, paths)
    else:
        assert paths["hash_plain"] == 0 and paths["hash_dma"] == 1, (stride, paths)
    c.close()


def test_ntt256_matches_oracle(torch, ctx, oracle):
    rng = np.random.default_rng(7)
    n = 1000 + 3  # not a multiple of 16 polynomials per workgroup
    a = rng.integers(-3328, 3329, size=(n, 256), dtype=np.int16)
    a[0] = 3328; a[1] = -3328; a[2] = 0           # extremes of the reference's input range
    a[3] = np.arange(256) % 3329
    d_in = _dev(torch, a)
    d_out = torch.zeros_like(d_in)
    torch.cuda.synchronize()  # torch fills / copies run on the null stream; the library streams are not ordered against it
    ctx.ntt256_batch(d_in.data_ptr(), d_out.data_ptr(), n)
    ctx.synchronize()
    out = d_out.cpu().numpy()
    for i in list(range(0, n, 37)) + [0, 1, 2, 3, n - 1]:
        assert np.array_equal(out[i], oracle.poly_ntt(a[i])), i
    bad = [i for i in range(n) if not np.array_equal(out[i], oracle.poly_ntt(a[i]))]   # every polynomial
    assert not bad, ("polynomials that differ from the oracle", len(bad), bad[:32])
    assert out.min() >= -1664 and out.max() <= 1664


def expand_exact(oracle, y):
    """oracle.recompute_shares on every row of y ([n][407] values in [0, q)): shares 0..150 are y[:, 256:407], shares 151..1453 the
    product with the oracle's share table mod q"""
    tab = oracle.table(0).astype(np.float64)                       # [1303][407]
    rest = np.mod(y.astype(np.float64) @ tab.T, 3329).astype(np.uint16)
    return np.concatenate([y[:, 256:407], rest], axis=1)


@pytest.mark.parametrize("n", [300, 9982])  # 9 982 rows = 46 proofs: every wave walks 10-11 table chunks (the pipelined epilogue's steady state)
def test_lagrange_expand_and_recon_match_oracle(n, torch, ctx, oracle):
    rng = np.random.default_rng(11)
    y = rng.integers(0, 3329, size=(n, 407), dtype=np.uint16)
    y[0] = 0; y[1] = 3328
    y[2] = 1664; y[3] = 1665  # the largest centred magnitudes: the limb products' sums are at their extremes for a constant row
    y[4, 0::2] = 1664; y[4, 1::2] = 1665
    y_in = y
    if n == 300:  # one row of values >= q: the folding conversion of the caller-data product
        y_in = y.copy()
        y_in[5] = _non_canonical(y[5])
        y[5] = y_in[5] % 3329
    d_y = _dev(torch, y_in)
    d_sh = torch.zeros((n, 1454), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()  # torch fills / copies run on the null stream; the library streams are not ordered against it
    ctx.lagrange_expand(d_y.data_ptr(), d_sh.data_ptr(), n)
    d_sec = torch.zeros((n, 256), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()  # torch fills / copies run on the null stream; the library streams are not ordered against it
    ctx.recon_secrets(d_sh.data_ptr(), d_sec.data_ptr(), n, False)
    ctx.synchronize()
    sh = d_sh.cpu().numpy().view(np.uint16)
    sec = d_sec.cpu().numpy().view(np.uint16)
    for i in list(range(0, n, 29 if n < 1000 else 499)) + [0, 1, 2, 3, 4, n - 1]:
        assert np.array_equal(sh[i], oracle.recompute_shares(y[i])), i
    # every row: the oracle's expansion as one exact float64 product (407 * 3328^2 < 2^53: every partial sum is an exact integer),
    # itself pinned against oracle.recompute_shares on the sampled rows first
    want = expand_exact(oracle, y)
    for i in (0, 1, 2, 3, 4, n // 2, n - 1):
        assert np.array_equal(want[i], oracle.recompute_shares(y[i])), i
    # shares 0..127 are points 256..383 of the row itself: no product writes them, a value >= q arrives as it was given
    assert np.array_equal(sh[:, :128], y_in[:, 256:384]) and np.array_equal(sh % 3329, want)
    bad = np.flatnonzero((sh[:, 128:] != want[:, 128:]).any(axis=1))
    assert not bad.size, ("rows that differ from the oracle's expansion", bad.size, bad[:32].tolist())
    # encode -> erase -> decode round trip on every row: the packed secrets come back
    assert np.array_equal(sec, y[:, :256])
    # degree-2d reconstruction of share-wise products = product of the packed secrets
    prod = (sh.astype(np.uint32)[0::2] * sh.astype(np.uint32)[1::2] % 3329).astype(np.uint16)
    if n == 300:
        # constant rows, the largest centred magnitudes (the limb sums of 13 k-steps at their extremes) and values >= q; 156 rows are
        # no multiple of 16: the last 48-row block is partial
        extra = np.zeros((6, 1454), dtype=np.uint16)
        extra[1] = 3328; extra[2] = 1664; extra[3] = 1665
        extra[4, 0::2] = 1664; extra[4, 1::2] = 1665
        extra[5] = _non_canonical(rng.integers(0, 3329, size=1454, dtype=np.uint16))
        prod = np.concatenate([prod, extra])
    d_p = _dev(torch, prod)
    d_s2 = torch.zeros((prod.shape[0], 256), dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()  # torch fills / copies run on the null stream; the library streams are not ordered against it
    ctx.recon_secrets(d_p.data_ptr(), d_s2.data_ptr(), prod.shape[0], True)
    ctx.synchronize()
    s2 = d_s2.cpu().numpy().view(np.uint16)
    exp = (y[0::2, :256].astype(np.uint32) * y[1::2, :256].astype(np.uint32) % 3329).astype(np.uint16)
    assert np.array_equal(s2[:exp.shape[0]], exp)
    assert np.array_equal(s2[3], oracle.recon(prod[3], True))
    for i in range(exp.shape[0], prod.shape[0]):
        assert np.array_equal(s2[i], oracle.recon(prod[i] % 3329, True)), i
    # all three tables (7 and 13 k-steps), caller data: every product ran on the table kernels
    paths = ctx.path_counts()
    assert paths["table_gemm"] > 0 and paths["limb_gemm"] == 0, paths
    if n == 300:
        _recon_2ddeg_two_chunks_per_wave(torch)


def _non_canonical(v):
    """values >= q for a conversion that folds: v + q (it always fits 16 bits), every fifth one 0xFFFF (another residue than v)"""
    out = v.astype(np.uint16) + np.uint16(3329)
    out[0::5] = 0xFFFF
    return out


def _recon_2ddeg_two_chunks_per_wave(torch):
    """7 680 rows = 160 blocks of 48 in ONE 13-k-step launch: the smallest product whose table is not split over workgroups, so
    that a wave walks two chunks and loads the second one's table fragments behind the first one's arithmetic.  A handle of 18
    proofs holds 18 x 435 = 7 830 rows."""
    from mpcith_kyber_kosk_amd import api
    m = 7680
    assert m % 48 == 0 and m // 48 == 160  # the launcher stops splitting the table at 160 row blocks
    y = np.random.default_rng(13).integers(0, 3329, size=(m + 1, 407), dtype=np.uint16)
    c = api.Kosk(kyber_k=3, max_batch=18)
    try:
        d_y = _dev(torch, y)
        d_sh = torch.zeros((m + 1, 1454), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()  # torch fills / copies run on the null stream; the library streams are not ordered against it
        c.lagrange_expand(d_y.data_ptr(), d_sh.data_ptr(), m + 1)
        c.synchronize()
        sh = d_sh.cpu().numpy().view(np.uint16).astype(np.uint32)
        d_p = _dev(torch, (sh[:-1] * sh[1:] % 3329).astype(np.uint16))  # overlapping pairs
        d_s2 = torch.zeros((m, 256), dtype=torch.int16, device="cuda")
        torch.cuda.synchronize()  # torch fills / copies run on the null stream; the library streams are not ordered against it
        before = c.path_counts()["table_gemm"]
        c.recon_secrets(d_p.data_ptr(), d_s2.data_ptr(), m, True)
        c.synchronize()
        assert c.path_counts()["table_gemm"] == before + 1, "the 7 680 rows must go in ONE launch (a chunked call has fewer than 160 blocks per launch)"
        s2 = d_s2.cpu().numpy().view(np.uint16)
    finally:
        c.close()
    y32 = y[:, :256].astype(np.uint32)
    assert np.array_equal(s2, (y32[:-1] * y32[1:] % 3329).astype(np.uint16))
