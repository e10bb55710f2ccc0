"""Caller-made inputs of kosk_prove_prepared / kosk_verify_inst: the reference's structs mpcith_randomness, mpcith_range_proof and
mlwe_inst (include/kosk_mi355x.h) written element by element, at contents no tape produces.  No GPU here: builders of the three byte
images from numpy arrays, their parsers, and the named catalogue.  Every case starts from the honest material of
oracle_lib.main_order(k, tape 31) and is proven on that tape's online slice; what a case expects is the oracle's prove() and
verify() on the same images (oracle_lib.prove_images, verify_inst_sites), made once per process and never changed."""
import ctypes as C
import functools

import numpy as np

from tests import oracle_lib as ol

Q, NSEC, NPARTY, NFREE = 3329, 256, 1454, 151  # 407 = 256 packed secrets + 151 free points define a degree-406 sharing
SHARE_VEC_BYTES = 8 + 4 * NPARTY
BASE_TAPE, OTHER_TAPE = 31, 32


# ---- images <-> arrays --------------------------------------------------------------------------------------------------------------
def share_vec(y, length=NPARTY, x=None):
    """share_vec { size_t len; u16 share_x[1454]; u16 share_y[1454]; }  (ss.hpp:33-37)"""
    x = np.arange(NPARTY, dtype=np.uint16) + NSEC if x is None else np.asarray(x, dtype=np.uint16)
    y = np.ascontiguousarray(y, dtype=np.uint16)
    assert y.shape == (NPARTY,) and x.shape == (NPARTY,)
    return int(length).to_bytes(8, "little") + x.tobytes() + y.tobytes()


def rand_image(f, ntt_f, f_sh, ntt_f_sh):
    """mpcith_randomness { u16 f[M][256]; u16 NTT_f[M][256]; share_vec f_shares[M], NTT_f_shares[M]; }  (mlwe_prover.hpp:39-44)"""
    f, ntt_f = (np.ascontiguousarray(a, dtype=np.uint16) for a in (f, ntt_f))
    assert f.shape == ntt_f.shape == (len(f_sh), NSEC) and len(ntt_f_sh) == len(f_sh)
    return f.tobytes() + ntt_f.tobytes() + b"".join(share_vec(y) for y in f_sh) + b"".join(share_vec(y) for y in ntt_f_sh)


def range_image(s_eta, e_eta):
    """mpcith_range_proof { share_vec s_eta_shares[K][2 eta1 + 1], e_eta_shares[K][2 eta1 + 1]; }: rows [i][j] as row i * E + j"""
    assert len(s_eta) == len(e_eta)
    return b"".join(share_vec(y) for y in s_eta) + b"".join(share_vec(y) for y in e_eta)


def inst_image(A, t, s, e):
    """mlwe_inst { polyvec A[K], t; polyvec s, e; } = i16 [K * K + 3 K][256]  (mlwe_prover.hpp:34-37)"""
    k = len(t)
    parts = [np.ascontiguousarray(a, dtype=np.int16) for a in (A, t, s, e)]
    assert parts[0].shape == (k, k, 256) and all(p.shape == (k, 256) for p in parts[1:])
    return b"".join(p.tobytes() for p in parts)


def _share_rows(img, n):
    a = np.frombuffer(img, dtype=np.uint8).reshape(n, SHARE_VEC_BYTES)
    return a[:, 8 + 2 * NPARTY:].copy().view(np.uint16).reshape(n, NPARTY)


def parse_rand(k, img):
    """-> f, NTT_f (M x 256), f_shares, NTT_f_shares (M x 1454 share_y), all u16 copies"""
    M = ol.params(k).M
    assert len(img) == M * (1024 + 2 * SHARE_VEC_BYTES)
    f = np.frombuffer(img[:M * 512], dtype=np.uint16).reshape(M, NSEC).copy()
    nf = np.frombuffer(img[M * 512:M * 1024], dtype=np.uint16).reshape(M, NSEC).copy()
    sh = _share_rows(img[M * 1024:], 2 * M)
    return f, nf, sh[:M], sh[M:]


def parse_range(k, img):
    """-> s_eta_shares, e_eta_shares (K * E x 1454 share_y)"""
    n = k * ol.params(k).E
    sh = _share_rows(img, 2 * n)
    return sh[:n], sh[n:]


def parse_inst(k, img):
    a = np.frombuffer(img, dtype=np.int16).reshape(k * k + 3 * k, 256).copy()
    return a[:k * k].reshape(k, k, 256), a[k * k:k * k + k], a[k * k + k:k * k + 2 * k], a[k * k + 2 * k:]


# ---- building blocks ----------------------------------------------------------------------------------------------------------------
def sharing(secrets, free):
    """the valid sharing (1454 share_y) of 256 packed secrets with the 151 free points given: recompute_share_secrets_ddeg"""
    y = np.empty(NSEC + NFREE, np.uint16)
    y[:NSEC] = secrets
    y[NSEC:] = free
    return ol.recompute_shares(y)


def constant_row(c):
    """the sharing whose polynomial is the constant c: secrets and free points all c"""
    return sharing(c, c)


def recon_rows(sh):
    """what recon_secrets_ddeg makes of each row: the packed secrets the reference's prove() works with"""
    return np.stack([ol.recon(y) for y in sh])


def mlwe_t(k, A, s, e):
    """t = A o NTT(s) + NTT(e) as kyber_keygen computes it (kosk.cpp:39-48), by the oracle's ring primitives"""
    lib = ol.lib
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    shat = np.stack([ol.poly_ntt(s[i]) for i in range(k)])
    ehat = np.stack([ol.poly_ntt(e[i]) for i in range(k)])
    t = np.zeros((k, 256), np.int16)
    for i in range(k):
        row = np.ascontiguousarray(A[i], dtype=np.int16)
        lib.ko_polyvec_basemul_acc(vp(t[i]), vp(row), vp(shat), k)
        lib.ko_poly_tomont(vp(t[i]))
        t[i] += ehat[i]
        lib.ko_poly_reduce(vp(t[i]))
    return t


@functools.lru_cache(maxsize=None)
def base(k, index=BASE_TAPE):
    """main_order on tape `index`: its images, its proof, and the slice of the tape that prove() consumes"""
    tape = ol.tape_bytes_for(k, index)
    ref = ol.main_order(k, tape)
    assert ref["verify"]
    u = ref["used"]
    return {"inst": ref["inst"], "rand": ref["rand"], "range": ref["range"], "tape": tape[u[2]:u[3]], "pi": ref["pi"]}


def largest_int16(a):
    """the largest int16 congruent to a mod q: a + 9 q where that fits, else a + 8 q"""
    a = np.asarray(a, dtype=np.int64)
    return (32767 - ((32767 - a) % Q)).astype(np.int16)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
def _with_rand(k, fn):
    b = base(k)
    f, nf, fs, nfs = parse_rand(k, b["rand"])
    out = fn(f, nf, fs, nfs)
    return dict(b, rand=rand_image(*out))


def _unread(value):
    def make(k):
        def fn(f, nf, fs, nfs):
            if value is None:  # the mask secrets of another tape
                f2, nf2, _, _ = parse_rand(k, base(k, OTHER_TAPE)["rand"])
                return f2, nf2, fs, nfs
            return np.full_like(f, value), np.full_like(nf, value), fs, nfs
        return _with_rand(k, fn)
    return make


def _whole(even, odd):
    def make(k):
        def fn(f, nf, fs, nfs):
            M = len(fs)
            rows = {c: constant_row(c) for c in (even, odd)}
            sh = np.stack([rows[even if i % 2 == 0 else odd] for i in range(M)])
            sec = np.stack([np.full(NSEC, even if i % 2 == 0 else odd, np.uint16) for i in range(M)])
            return sec, sec.copy(), sh, sh.copy()
        return _with_rand(k, fn)
    return make


def _single(row):
    def make(k):
        def fn(f, nf, fs, nfs):
            r = row if row >= 0 else len(fs) + row
            for sec, sh in ((f, fs), (nf, nfs)):
                sec[r] = 1665
                sh[r] = constant_row(1665)
            return f, nf, fs, nfs
        return _with_rand(k, fn)
    return make


def _not_a_sharing(k):
    def fn(f, nf, fs, nfs):
        rng = np.random.default_rng(270000 + k)
        M = len(fs)
        sh = rng.integers(0, Q, size=(2 * M, NPARTY), dtype=np.uint16)
        junk = rng.integers(0, 65536, size=(2 * M, NSEC), dtype=np.uint16)
        return junk[:M], junk[M:], sh[:M], sh[M:]
    return _with_rand(k, fn)


def _unrelated_halves(k):
    return _with_rand(k, lambda f, nf, fs, nfs: (f, f.copy(), fs, fs.copy()))


def _range(free):
    def make(k):
        b = base(k)
        p = ol.params(k)
        rng = np.random.default_rng(270100 + k)
        rows = []
        for q in range(2 * k * p.E):
            cst = (q % p.E - p.eta1) % Q   # encode_to_gf3329(m - eta1)   mlwe_prover.cpp:47-50
            rows.append(sharing(cst, rng.integers(0, Q, size=NFREE, dtype=np.uint16) if free is None else free))
        n = k * p.E
        return dict(b, range=range_image(rows[:n], rows[n:]))
    return make


def _with_inst(k, fn):
    b = base(k)
    return dict(b, inst=inst_image(*fn(*parse_inst(k, b["inst"]))))


def _se(kind):
    def make(k):
        def fn(A, t, s, e):
            eta1 = ol.params(k).eta1
            for v in (s, e):
                if kind == "one_eta":
                    v[:] = 0
                    v[k - 1, 255] = eta1
                elif kind == "alt":
                    v[:] = 1664
                    v[:, 1::2] = -1664
                else:
                    v[:] = kind
            return A, mlwe_t(k, A, s, e), s, e   # t follows s and e: the relation holds, only the range may not
        return _with_inst(k, fn)
    return make


def _A(kind):
    def make(k):
        def fn(A, t, s, e):
            assert A.min() >= 0 and A.max() < Q
            A2 = largest_int16(A) if kind == "max" else (A.astype(np.int32) + kind * Q).astype(np.int16)
            return A2, t, s, e
        return _with_inst(k, fn)
    return make


def _t_junk(k):
    def fn(A, t, s, e):
        junk = np.random.default_rng(270200 + k).integers(-32768, 32768, size=t.shape).astype(np.int16)
        return A, junk, s, e
    return _with_inst(k, fn)


SINGLE_ROWS = (0, 63, 64, 70, 71, -1)   # base term; the k-step boundary; last check row; the r rows' constant term; last live row
CATALOGUE = {
    "honest": base,
    # members prove() does not read (mlwe_prover.cpp: f and NTT_f occur in prepare_randomness and the struct copy only)
    "unread_0": _unread(0), "unread_3328": _unread(3328), "unread_ffff": _unread(0xFFFF), "unread_other_tape": _unread(None),
    # all 2M share rows constant, f and NTT_f equal to their reconstruction
    "all_0": _whole(0, 0), "all_3328": _whole(3328, 3328), "all_1664": _whole(1664, 1664), "all_1665": _whole(1665, 1665),
    "even_1664_odd_1665": _whole(1664, 1665),
    # one row pair (f_k, NTT f_k) constant 1665 in the honest matrix
    "row_0": _single(0), "row_63": _single(63), "row_64": _single(64), "row_70": _single(70), "row_71": _single(71), "row_last": _single(-1),
    "not_a_sharing": _not_a_sharing,
    "unrelated_halves": _unrelated_halves,
    "range_free_0": _range(0), "range_free_3328": _range(3328), "range_free_uniform": _range(None),
    "se_3328": _se(3328), "se_minus_3328": _se(-3328), "se_alt_1664": _se("alt"), "se_one_eta1": _se("one_eta"),
    "A_minus_q": _A(-1), "A_plus_8q": _A(8), "A_largest_int16": _A("max"),
    "t_junk": _t_junk,
}
NAMES = tuple(CATALOGUE)
FEW = ("honest", "unread_0", "all_1665", "row_71", "row_last", "not_a_sharing", "A_minus_q")   # K = 2 and K = 4
UNREAD = ("unread_0", "unread_3328", "unread_ffff", "unread_other_tape")
WHOLE = ("all_0", "all_3328", "all_1664", "all_1665", "even_1664_odd_1665")
SINGLE = ("row_0", "row_63", "row_64", "row_70", "row_71", "row_last")
RANGE = ("range_free_0", "range_free_3328", "range_free_uniform")


def names(k):
    return NAMES if k == 3 else FEW


@functools.lru_cache(maxsize=None)
def case(k, name):
    """{"inst", "rand", "range", "tape"} (byte images) of a catalogue case"""
    c = CATALOGUE[name](k)
    return {key: c[key] for key in ("inst", "rand", "range", "tape")}


@functools.lru_cache(maxsize=None)
def expected(k, name):
    """(pi, verify bit, sites) of the oracle on the case's images: prove(), then verify() of that proof against the same instance"""
    c = case(k, name)
    pi = ol.prove_images(k, c["inst"], c["rand"], c["range"], c["tape"])
    bit, sites = ol.verify_inst_sites(k, pi, c["inst"])
    return pi, bit, tuple(sites)


def expected_all(k):
    """expected() of every case of names(k), made on eight threads (the oracle's prove and verify hold no state once its tables exist,
    which the first, single-threaded case sees to; ctypes calls run without the interpreter lock)"""
    from concurrent.futures import ThreadPoolExecutor
    ns = names(k)
    out = {ns[0]: expected(k, ns[0])}
    with ThreadPoolExecutor(max_workers=8) as pool:
        out.update(zip(ns[1:], pool.map(lambda name: expected(k, name), ns[1:])))
    return out


def mask_of(sites):
    """the fail mask a verifier that runs every check reports: bit b set where sites[b] comparisons failed"""
    return sum(1 << b for b, n in enumerate(sites) if n)
