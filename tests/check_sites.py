"""Tampered proofs that break ONE comparison of ONE check of the verifier and leave every hash alone.  Tests only; it calls nothing of
the library (the oracle only for the layout of the image and, in expected(), for its verdicts).

The verifier recomputes hashes only over the opened parties' s, e, f, NTT f, the first K of beta / gamma as computed, s + r and e + r at
opened points as interpolated, z_s, z_e and u at opened points.  It hashes neither the opened records of NTT(s), NTT(e), NTT(Ar),
NTT(As) (fields 9-12) nor any share field of the unopened parties (2, 3, 8, 13-16, 21, 22): a tamper there leaves I' == I (fail bit 11
clear), and what it breaks is decided by the relation checks alone, fail bits 1-10 of DESIGN.md section 4.

Arithmetic is mod q = 3329.  Secret c is the point x = c, party p the point x = 256 + p.  `rest` is the unopened parties ascending; the
nodes of the degree-d interpolation are rest[0:407], those of degree 2d rest[0:813].  A "D tamper" adds D(x) = prod_{z in Z} (x - z)
to a field's node records: deg D <= d (2d), so the interpolated polynomial moves by D itself, which is zero on Z -- with Z all secrets
but c* (all opened parties but the j*-th) exactly one interpolated secret (one recomputed opened share) moves.  A "plain tamper" adds
d to one opened record of fields 9-12, which enter three comparisons only: NTT(s) = .. (9), NTT(e) = .. (10), A(s+r) = NTT(As) +
NTT(Ar) (11, 12) and t = NTT(As) + NTT(e) (12, 10); a second and third record restore the comparisons that are not meant to break.

Every case sits at the edges of its index space: polynomial i in {0, K-1}, secret c* in {0, 255} (63 / 64 once per check), opened
position j* in {0, 149} (64 once), the s and the e side, gate m in {0, E-1}, z in {0, Z-1}, beta / gamma column in {0, 69}, positions
407, 1279, 1280, 1303 of `rest` for the s + r / e + r comparison (the first record behind the nodes, the last of a full block of 256,
the first of the ragged block, the last record)."""
import numpy as np

Q = 3329
NPARTY, NOPEN, NSEC, DEG, DEG2, NCHK = 1454, 150, 256, 406, 812, 70
NREST = NPARTY - NOPEN
# field ids of the image (oracle/kosk_oracle.h)
F_BETA, F_GAMMA, F_I, F_T, F_NTTS, F_NTTE, F_NTTAR, F_NTTAS, F_SR, F_ER, F_SETA, F_EETA, F_US, F_UE = 2, 3, 5, 8, 9, 10, 11, 12, 13, 14, 15, 16, 21, 22
DELTA = 1  # the d of a plain tamper: any non-zero residue

L = "L"  # "the last one": K - 1, E - 1, Z - 1, resolved per K by case()

# row -> (intended fail bits, intended number of failing sites or None = many, parameter names, corners).  The first two corners
# of a row are its two extremes (all-low, all-high): they run at every K; the others run at K = 3 only.
ROWS = {
    "gamma": ((1,), 1, ("col", "c"), [(0, 0), (69, 255), (0, 255), (69, 0), (0, 63)]),
    "beta": ((1,), None, ("col", "c"), [(0, 0), (69, 255), (69, 64), (0, 255)]),
    "sr_er": ((2,), 1, ("side", "i", "pos"), [("s", 0, 407), ("e", L, 1303), ("s", L, 1279), ("e", 0, 1280), ("s", 0, 1303), ("e", L, 407)]),
    "ntt_s": ((3,), 1, ("i", "j"), [(0, 0), (L, 149), (0, 149), (L, 0), (1, 64)]),
    "ntt_e": ((3,), 1, ("i", "j"), [(0, 0), (L, 149), (0, 149), (L, 0), (1, 64)]),
    "a_sr": ((4,), 1, ("i", "j"), [(0, 0), (L, 149), (0, 149), (L, 0), (1, 64)]),
    "t_rel": ((6,), 1, ("i", "j"), [(0, 0), (L, 149), (0, 149), (L, 0), (1, 64)]),
    "t_rel_tside": ((6,), 1, ("i", "j"), [(0, 0), (L, 149), (0, 149), (L, 0), (1, 64)]),
    "t_pk": ((5,), 1, ("i", "c"), [(0, 0), (L, 255), (0, 255), (L, 0), (1, 63)]),
    "t_pk_pkside": ((5,), 1, ("i", "c"), [(0, 0), (L, 255), (0, 255), (L, 0), (1, 64)]),
    "eta": ((7,), 1, ("side", "i", "m", "c"), [("s", 0, 0, 0), ("e", L, L, 255), ("s", L, L, 0), ("e", 0, 0, 255), ("s", 0, L, 255),
                                              ("e", L, 0, 0), ("s", 1, 1, 64)]),
    "sub_eta": ((8,), 1, ("side", "i", "m", "j"), [("s", 0, 0, 0), ("e", L, L, 149), ("s", L, L, 0), ("e", 0, 0, 149), ("s", 0, L, 149),
                                                  ("e", L, 0, 0), ("e", 1, 1, 64)]),
    "u_interp": ((9, 10), (1, 1), ("side", "i", "z", "c"), [("s", 0, 0, 0), ("e", L, L, 255), ("s", L, L, 0), ("e", 0, 0, 255),
                                                            ("s", 0, L, 255), ("e", L, 0, 0), ("e", 1, 1, 63)]),
    "u_recon": ((10,), None, ("side", "i", "z"), [("s", 0, 0), ("e", L, L), ("s", L, L), ("e", 0, 0)]),
    "two_ntte": ((3, 6), (1, 1), ("i", "j"), [(0, 0), (L, 149)]),
    "two_nttas": ((4, 6), (1, 1), ("i", "j"), [(0, 0), (L, 149)]),
}


def _name(row, corner):
    return row + ":" + ",".join("%s=%s" % (n, v) for n, v in zip(ROWS[row][2], corner))


# name -> (intended bits, intended site count per bit or None)
CATALOGUE = {}
_CORNER = {}
for _row, (_bits, _count, _pn, _corners) in ROWS.items():
    for _n, _c in enumerate(_corners):
        _cnt = None if _count is None else (_count,) * len(_bits) if isinstance(_count, int) else _count
        CATALOGUE[_name(_row, _c)] = (_bits, _cnt)
        _CORNER[_name(_row, _c)] = (_row, _c, _n < 2)


def names(k):
    """the cases that run at this K: every one at K = 3, the two extreme corners of every row at K = 2 and K = 4"""
    return [n for n, (_, _, extreme) in _CORNER.items() if k == 3 or extreme]


def intended_mask(name):
    return sum(1 << b for b in CATALOGUE[name][0])


def is_pk_case(name):
    return _CORNER[name][0] == "t_pk_pkside"


_PARAMS = {}


def _params(k):
    if k not in _PARAMS:
        from tests import oracle_lib
        p = oracle_lib.params(k)
        _PARAMS[k] = {"E": p.E, "Z": p.Z, "off": list(p.off), "size": list(p.size)}
    return _PARAMS[k]


def opened_and_rest(k, pi):
    o = _params(k)["off"][F_I]
    I = [int.from_bytes(pi[o + 2 * i:o + 2 * i + 2], "little") for i in range(NOPEN)]
    assert len(set(I)) == NOPEN and max(I) < NPARTY
    opened = set(I)
    return I, [p for p in range(NPARTY) if p not in opened]


def D(zeros, xs):
    """prod_{z in zeros} (x - z) mod q at every x of xs"""
    x = np.asarray(xs, dtype=np.int64)
    acc = np.ones(len(x), dtype=np.int64)
    for z in zeros:
        acc = acc * (x - z) % Q
    return [int(v) for v in acc]


class _Image:
    def __init__(self, k, pi):
        self.b, self.off = bytearray(pi), _params(k)["off"]

    def add(self, field, index, delta):
        o = self.off[field] + 2 * index
        v = int.from_bytes(self.b[o:o + 2], "little")
        assert v < Q  # an honest proof holds canonical residues, and so does every tampered one
        self.b[o:o + 2] = ((v + delta) % Q).to_bytes(2, "little")


def case(k, pi, name):
    """the tampered image of the catalogue's case `name` from the honest proof pi (for a pk-side case: the proof itself, see case_pk)"""
    row, corner, _ = _CORNER[name]
    P = _params(k)
    E, Z = P["E"], P["Z"]
    a = dict(zip(ROWS[row][2], corner))
    last = {"i": k - 1, "m": E - 1, "z": Z - 1}
    for n in a:
        if a[n] == L:
            a[n] = last[n]
    i, j, c = a.get("i"), a.get("j"), a.get("c")
    assert i is None or 0 <= i < k
    I, rest = opened_and_rest(k, pi)
    secrets, parties = list(range(NSEC)), [NSEC + p for p in I]
    img = _Image(k, pi)

    def add_D(field, width, col, zeros, nodes):
        """D over the field's records of the unopened parties `nodes` (positions in rest), record k = row k of `width` columns"""
        assert len(zeros) == len(set(zeros)) and len(zeros) <= (DEG if len(nodes) <= DEG + 1 else DEG2)
        for kk, d in zip(nodes, D(zeros, [NSEC + rest[kk] for kk in nodes])):
            img.add(field, kk * width + col, d)

    if row in ("gamma", "beta"):
        # the reconstruction reads parties 0..406: the unopened ones from the image, the opened ones from f / NTT f (hashed)
        nodes = [kk for kk in range(NREST) if rest[kk] <= DEG]
        zeros = [s for s in secrets if s != c] + [NSEC + p for p in I if p <= DEG]
        add_D(F_GAMMA if row == "gamma" else F_BETA, NCHK, a["col"], zeros, nodes)
    elif row == "sr_er":
        assert a["pos"] > DEG
        img.add(F_SR if a["side"] == "s" else F_ER, a["pos"] * k + i, 1)
    elif row == "ntt_s":
        img.add(F_NTTS, j * k + i, DELTA)
    elif row == "ntt_e":
        img.add(F_NTTE, j * k + i, DELTA)
        img.add(F_NTTAS, j * k + i, -DELTA)
        img.add(F_NTTAR, j * k + i, DELTA)
    elif row == "a_sr":
        img.add(F_NTTAR, j * k + i, DELTA)
    elif row == "t_rel":
        img.add(F_NTTAS, j * k + i, DELTA)
        img.add(F_NTTAR, j * k + i, -DELTA)
    elif row == "t_rel_tside":
        add_D(F_T, k, i, secrets + [x for n, x in enumerate(parties) if n != j], range(DEG + 1))
    elif row == "t_pk":
        add_D(F_T, k, i, [s for s in secrets if s != c] + parties, range(DEG + 1))
    elif row == "t_pk_pkside":
        pass
    elif row == "eta":
        add_D(F_SETA if a["side"] == "s" else F_EETA, k * E, i * E + a["m"], [s for s in secrets if s != c] + parties, range(DEG + 1))
    elif row == "sub_eta":
        add_D(F_SETA if a["side"] == "s" else F_EETA, k * E, i * E + a["m"], secrets + [x for n, x in enumerate(parties) if n != j],
              range(DEG + 1))
    elif row == "u_interp":
        # the reconstruction reads parties 0..812, every unopened one of them a node: D is zero on the opened ones among them
        zeros = [s for s in secrets if s != c] + [NSEC + p for p in I if p <= DEG2]
        add_D(F_US if a["side"] == "s" else F_UE, k * Z, i * Z + a["z"], zeros, range(DEG2 + 1))
    elif row == "u_recon":
        add_D(F_US if a["side"] == "s" else F_UE, k * Z, i * Z + a["z"], secrets, range(DEG2 + 1))
    elif row == "two_ntte":
        img.add(F_NTTE, j * k + i, DELTA)
    elif row == "two_nttas":
        img.add(F_NTTAS, j * k + i, DELTA)
    else:
        raise KeyError(name)
    return bytes(img.b)


def case_pk(k, pk, name):
    """the public key of the case: the honest one, except for the pk-side case of t != pk: 12-bit field (i, c*) of t-hat += 1 mod q"""
    if not is_pk_case(name):
        return pk
    _, corner, _ = _CORNER[name]
    i, c = (k - 1 if v == L else v for v in corner)
    b = bytearray(pk)
    o = 384 * i + 3 * (c // 2)
    two = int.from_bytes(b[o:o + 3], "little")            # coefficients 2n, 2n + 1 (poly_tobytes, poly.c)
    t = [two & 0xFFF, two >> 12]
    assert t[c % 2] < Q
    t[c % 2] = (t[c % 2] + 1) % Q
    b[o:o + 3] = (t[0] | t[1] << 12).to_bytes(3, "little")
    return bytes(b)


_EXPECTED = {}


def expected(oracle, k, cases):
    """cases = [(pi, pk)] -> [(mask, sites)] by ko_kosk_verify_sites: mask = OR(1 << b for sites[b] > 0).  A few at a time (ctypes
    releases the interpreter lock, the counts travel through the call's own out-parameter); cached per process by content."""
    from concurrent.futures import ThreadPoolExecutor
    import hashlib
    keys = [(k, hashlib.sha256(pi).digest(), hashlib.sha256(pk).digest()) for pi, pk in cases]
    todo = {key: c for key, c in zip(keys, cases) if key not in _EXPECTED}
    if todo:
        first = next(iter(todo.values()))
        oracle.kosk_verify_sites(k, *first)  # the oracle's tables are built here, by one thread
        with ThreadPoolExecutor(6) as ex:
            got = list(ex.map(lambda c: oracle.kosk_verify_sites(k, *c), todo.values()))
        for key, (ok, sites) in zip(todo, got):
            mask = sum(1 << b for b in range(12) if sites[b])
            assert ok == (mask == 0)
            _EXPECTED[key] = (mask, sites)
    return [_EXPECTED[key] for key in keys]


TAPE_INDEX = 2300  # the fixed tape of the catalogue's honest proof, per K (oracle_lib.tape_bytes_for)
_BUILT = {}


def build(oracle, k):
    """{"honest": (pk, pi), "cases": {name: (pk, pi)}} on the oracle's own proof of the fixed tape; cached per process"""
    if k not in _BUILT:
        pk, _, pi = oracle.verifiable_keygen(k, oracle.tape_bytes_for(k, TAPE_INDEX))[:3]
        _BUILT[k] = {"honest": (pk, pi), "cases": {n: (case_pk(k, pk, n), case(k, pi, n)) for n in names(k)}}
    return _BUILT[k]
