"""Host (no GPU): the oracle side of the caller-made struct tests (tests/split_structs.py, tests/test_gpu_27_split_structs.py) --
ko_pre_from_images, the catalogue's shapes, and what the reference semantics make of every case.

What the oracle decides, written down (K = 3; the K = 2 and K = 4 subsets agree):
  accepted   honest; the four cases that differ in f / NTT_f only (prove() never reads them: the proof bytes are the honest ones);
             all_0; the three range cases; A - q, A + 8q, the largest int16 representatives (the proof bytes are the honest ones: A
             enters through fqmul only); and the four s / e cases, 3328, -3328 and +-1664 included: encode_to_gf3329 maps them to
             field elements, t was recomputed from them, and the reference's verifier checks the multiplication gates of the range
             product (checks 8-10) but never that the last product is zero, so nothing it looks at depends on the range of s and e.
  rejected   every case with a constant non-zero f row next to a constant NTT f row (the whole-matrix extremes but 0, the single
             rows): a constant vector c is not the NTT of the constant polynomial c, so check 1, NTT(beta_j) = gamma_j, fails at
             every j -- the prover does not care, the verifier has to.  The same for unrelated halves and for rows that are no
             sharing; the latter also fails the checks on the 1 304 unopened shares (2, 3, 4, 6) and the opened set (11), whose
             hash input is recomputed from the first 407 parties.  t junk: the proof is the honest one, check 5 (t itself) fails alone.
The GPU test compares bit and mask with these per case; nothing here is typed in but the classes."""

import numpy as np
import pytest

from tests import oracle_lib as ol
from tests import split_structs as ss

Q = ss.Q
ACCEPT = ("honest",) + ss.UNREAD + ("all_0",) + ss.RANGE + ("se_3328", "se_minus_3328", "se_alt_1664", "se_one_eta1",
                                                           "A_minus_q", "A_plus_8q", "A_largest_int16")
REJECT_CHECK1 = tuple(n for n in ss.WHOLE if n != "all_0") + ss.SINGLE + ("not_a_sharing", "unrelated_halves")
SAME_PROOF = ss.UNREAD + ("A_minus_q", "A_plus_8q", "A_largest_int16", "t_junk")


def test_catalogue_is_complete():
    assert len(ss.NAMES) == 29 and set(ss.FEW) <= set(ss.NAMES)
    assert sorted(ACCEPT + REJECT_CHECK1 + ("t_junk",)) == sorted(ss.NAMES)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_images_reproduce_main_order(k):
    b = ss.base(k)
    assert ol.prove_images(k, b["inst"], b["rand"], b["range"], b["tape"]) == b["pi"]
    assert ss.expected(k, "honest") == (b["pi"], True, (0,) * 12)
    # the builders are the inverse of the parsers on the oracle's own images
    assert ss.rand_image(*ss.parse_rand(k, b["rand"])) == b["rand"]
    assert ss.range_image(*ss.parse_range(k, b["range"])) == b["range"]
    assert ss.inst_image(*ss.parse_inst(k, b["inst"])) == b["inst"]
    assert ol.mlwe_inst_bytes(k, ol.mlwe_from_inst_bytes(k, b["inst"])) == b["inst"]
    A, t, s, e = ss.parse_inst(k, b["inst"])
    assert (ss.mlwe_t(k, A, s, e) == t).all()


def test_pre_from_images_refuses_len_and_share_x():
    k = 3
    b = ss.base(k)
    M, E = ol.params(k).M, ol.params(k).E
    pre = ol.lib.ko_pre_alloc()
    try:
        assert ol.pre_from_images(k, pre, b["rand"], b["range"]) == 0
        first = M * 1024                                        # f_shares[0]
        last = M * 1024 + (2 * M - 1) * ss.SHARE_VEC_BYTES      # NTT_f_shares[M - 1]
        for off in (first, last):
            for patch in ((0, (1453).to_bytes(8, "little")), (0, (1455).to_bytes(8, "little")), (0, (1454 + (1 << 32)).to_bytes(8, "little")),
                          (8, (255).to_bytes(2, "little")), (8 + 2 * 1453, (256 + 1452).to_bytes(2, "little"))):
                img = bytearray(b["rand"])
                img[off + patch[0]:off + patch[0] + len(patch[1])] = patch[1]
                assert ol.pre_from_images(k, pre, bytes(img), b["range"]) == -1, (off, patch)
        for row in (0, 2 * k * E - 1):
            off = row * ss.SHARE_VEC_BYTES
            for patch in ((0, (0).to_bytes(8, "little")), (8 + 2 * 700, (700).to_bytes(2, "little"))):
                img = bytearray(b["range"])
                img[off + patch[0]:off + patch[0] + len(patch[1])] = patch[1]
                assert ol.pre_from_images(k, pre, b["rand"], bytes(img)) == -1, (row, patch)
    finally:
        ol.lib.ko_pre_free(pre)


def test_pre_from_images_copies_values_as_they_are():
    k = 2
    p = ol.params(k)
    rng = np.random.default_rng(2700)
    M, n = p.M, k * p.E
    f, nf = (rng.integers(0, 65536, size=(M, 256), dtype=np.uint16) for _ in range(2))
    fs, nfs = (rng.integers(0, 65536, size=(M, ss.NPARTY), dtype=np.uint16) for _ in range(2))
    se, ee = (rng.integers(0, 65536, size=(n, ss.NPARTY), dtype=np.uint16) for _ in range(2))
    pre = ol.lib.ko_pre_alloc()
    try:
        assert ol.pre_from_images(k, pre, ss.rand_image(f, nf, fs, nfs), ss.range_image(se, ee)) == 0
        arr = lambda ptr, m: np.ctypeslib.as_array(ptr, shape=(m,))
        for i in range(M):
            assert (arr(ol.lib.ko_pre_f(pre, i), 256) == f[i]).all() and (arr(ol.lib.ko_pre_ntt_f(pre, i), 256) == nf[i]).all()
            assert (arr(ol.lib.ko_pre_f_shares(pre, i), ss.NPARTY) == fs[i]).all()
            assert (arr(ol.lib.ko_pre_ntt_f_shares(pre, i), ss.NPARTY) == nfs[i]).all()
        for i in range(k):
            for j in range(p.E):
                assert (arr(ol.lib.ko_pre_s_eta_shares(pre, i, j), ss.NPARTY) == se[i * p.E + j]).all()
                assert (arr(ol.lib.ko_pre_e_eta_shares(pre, i, j), ss.NPARTY) == ee[i * p.E + j]).all()
    finally:
        ol.lib.ko_pre_free(pre)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_unread_members_leave_the_proof_alone(k):
    """prove() never reads rand->f or rand->NTT_f: whatever they hold, the oracle's proof is the honest one, and it verifies"""
    b = ss.base(k)
    for name in ss.UNREAD:
        c = ss.CATALOGUE[name](k)
        f, nf, fs, nfs = ss.parse_rand(k, c["rand"])
        f0, nf0, fs0, nfs0 = ss.parse_rand(k, b["rand"])
        assert (fs == fs0).all() and (nfs == nfs0).all() and (f != f0).any() and (nf != nf0).any(), name
        pi = ol.prove_images(k, c["inst"], c["rand"], c["range"], c["tape"])
        assert pi == b["pi"], (k, name)
    assert ol.verify_inst_sites(k, b["pi"], b["inst"]) == (True, [0] * 12)


def _valid(row):
    """a row of 1454 share_y lies on one degree-406 polynomial: parties 407.. follow from recon_secrets_ddeg and parties 0..150"""
    y = np.concatenate([ol.recon(row), row[:ss.NFREE]])
    return (ol.recompute_shares(y) == row).all()


def test_shapes_of_the_randomness_cases():
    k = 3
    M = ol.params(k).M
    f0, nf0, fs0, nfs0 = ss.parse_rand(k, ss.base(k)["rand"])
    assert all(_valid(r) for r in fs0[:3]) and _valid(nfs0[M - 1])           # the control: honest rows are sharings
    for name, even, odd in (("all_0", 0, 0), ("all_3328", 3328, 3328), ("all_1664", 1664, 1664), ("all_1665", 1665, 1665),
                            ("even_1664_odd_1665", 1664, 1665)):
        f, nf, fs, nfs = ss.parse_rand(k, ss.case(k, name)["rand"])
        for i in range(M):
            c = odd if i % 2 else even
            for sec, sh in ((f, fs), (nf, nfs)):
                assert (sh[i] == c).all() and (sec[i] == c).all(), (name, i)   # constant over all 1454 parties, f consistent
        assert (ss.recon_rows(fs[:2]) == f[:2]).all()
    for name, row in zip(ss.SINGLE, ss.SINGLE_ROWS):
        r = row if row >= 0 else M + row
        f, nf, fs, nfs = ss.parse_rand(k, ss.case(k, name)["rand"])
        others = np.arange(M) != r
        for got, base in ((f, f0), (nf, nf0), (fs, fs0), (nfs, nfs0)):
            assert (got[r] == 1665).all() and (got[others] == base[others]).all(), name
    assert [r if r >= 0 else M + r for r in ss.SINGLE_ROWS] == [0, 63, 64, 70, 71, M - 1]
    f, nf, fs, nfs = ss.parse_rand(k, ss.case(k, "not_a_sharing")["rand"])
    assert fs.max() < Q and nfs.max() < Q and f.max() >= Q and nf.max() >= Q
    assert not any(_valid(r) for r in list(fs) + list(nfs))
    assert len({r.tobytes() for r in list(fs) + list(nfs)}) == 2 * M
    f, nf, fs, nfs = ss.parse_rand(k, ss.case(k, "unrelated_halves")["rand"])
    assert (fs == fs0).all() and (nfs == fs0).all() and (f == f0).all() and (nf == f0).all()


@pytest.mark.parametrize("k", [2, 3, 4])
def test_shapes_of_the_range_cases(k):
    p = ol.params(k)
    seen = []
    for name, free in zip(ss.RANGE, (0, 3328, None)):
        rows = np.concatenate(ss.parse_range(k, ss.CATALOGUE[name](k)["range"]))
        assert rows.shape == (2 * k * p.E, ss.NPARTY) and rows.max() < Q
        for q, row in enumerate(rows):
            assert (ol.recon(row) == (q % p.E - p.eta1) % Q).all(), (name, q)   # reconstructs to the constant m - eta1
            assert _valid(row), (name, q)
            if free is not None:
                assert (row[:ss.NFREE] == free).all()
        seen.append(rows.tobytes())
    assert len(set(seen + [ss.base(k)["range"]])) == 4


def test_shapes_of_the_instance_cases():
    k = 3
    eta1 = ol.params(k).eta1
    A0, t0, s0, e0 = ss.parse_inst(k, ss.base(k)["inst"])
    assert A0.min() >= 0 and A0.max() < Q and abs(s0).max() <= eta1 and abs(e0).max() <= eta1
    for name, lo, hi in (("se_3328", 3328, 3328), ("se_minus_3328", -3328, -3328), ("se_alt_1664", -1664, 1664), ("se_one_eta1", 0, eta1)):
        A, t, s, e = ss.parse_inst(k, ss.case(k, name)["inst"])
        assert (A == A0).all() and s.min() == lo and s.max() == hi and (e == s).all() and (t == ss.mlwe_t(k, A, s, e)).all(), name
    A, t, s, e = ss.parse_inst(k, ss.case(k, "se_alt_1664")["inst"])
    assert (s[:, 0::2] == 1664).all() and (s[:, 1::2] == -1664).all()
    A, t, s, e = ss.parse_inst(k, ss.case(k, "se_one_eta1")["inst"])
    assert np.count_nonzero(s) == 1 and s[k - 1, 255] == eta1
    for name, check in (("A_minus_q", lambda A: A.max() < 0), ("A_plus_8q", lambda A: A.min() >= 8 * Q),
                        ("A_largest_int16", lambda A: A.min() > 32767 - Q and A.flat[A0.argmax()] == 32767 - (32767 - int(A0.max())) % Q
                         and (A >= 9 * Q).any() and (A < 9 * Q).any())):
        A, t, s, e = ss.parse_inst(k, ss.case(k, name)["inst"])
        assert check(A) and ((A.astype(np.int32) - A0) % Q == 0).all() and (t == t0).all() and (s == s0).all() and (e == e0).all(), name
    A, t, s, e = ss.parse_inst(k, ss.case(k, "t_junk")["inst"])
    assert (A == A0).all() and (s == s0).all() and (t != t0).any() and t.min() < -Q and t.max() > Q


def test_everything_else_is_canonical():
    k = 3
    for name in ss.NAMES:
        c = ss.case(k, name)
        f, nf, fs, nfs = ss.parse_rand(k, c["rand"])
        assert fs.max() < Q and nfs.max() < Q and np.concatenate(ss.parse_range(k, c["range"])).max() < Q, name
        if name not in ("unread_ffff", "not_a_sharing"):
            assert f.max() < Q and nf.max() < Q, name
        A, t, s, e = ss.parse_inst(k, c["inst"])
        assert abs(s).max() < Q and abs(e).max() < Q, name
        if not name.startswith("A_"):
            assert A.min() >= 0 and A.max() < Q, name
        assert c["tape"] == ss.base(k)["tape"]


@pytest.mark.parametrize("k", [2, 3, 4])
def test_verdict_classes(k):
    honest = ss.base(k)["pi"]
    for name, (pi, bit, sites) in ss.expected_all(k).items():
        mask = ss.mask_of(sites)
        assert bit == (mask == 0), name
        assert (pi == honest) == (name == "honest" or name in SAME_PROOF), name
        if name in ACCEPT:
            assert bit, (k, name, sites)
        elif name in REJECT_CHECK1:
            assert not bit and sites[1] > 0 and sites[0] == 0, (k, name, sites)
            if name != "not_a_sharing":
                assert not mask & ~((1 << 1) | (1 << 5)), (k, name, sites)   # the proof's own shares are consistent: no other check fails
        else:
            assert name == "t_junk" and mask == 1 << 5, (k, name, sites)
