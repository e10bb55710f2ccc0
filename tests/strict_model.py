"""Which u16 records of a proof image the reference's verifier reads -- the read set the strict default checks.

Restated from the reference's line numbers alone, never from the library's sources:

  * the records of the 150 OPENED parties (fields 0, 1, 6, 7, 9, 10, 11, 12, 17, 18, 19, 20) are all hashed and compared;
  * s + r / e + r shares (13, 14) of EVERY unopened party are compared with the recomputed shares, mlwe_verifier.cpp:232-246;
  * beta / gamma shares (2, 3) only enter recon_secrets_ddeg, which takes the shares of PARTIES 0 .. 406 (:106-107): record i of
    the 1 304 unopened parties is read iff rest[i] < 407;
  * t (8) and eta (15, 16) shares only serve as interpolation nodes, the first 407 unopened parties (:321-323, :390-394): read iff
    i < 407, whichever party that is;
  * u shares (21, 22): nodes are the first 813 unopened parties (:503-507) and recon_secrets_2ddeg takes parties 0 .. 812
    (:555-556); an unopened party below 813 is among the first 813 unopened ones, so: read iff i < 813.

Helper of tests/test_strict_model.py (which pins this model to the oracle, position by position) and of
tests/test_gpu_15_strict_encoding.py (which takes every expectation from here)."""
import functools

import numpy as np

Q = 3329
NPARTY, NOPEN = 1454, 150
NREST = NPARTY - NOPEN
BYTE_FIELDS = (4, 23)  # Tcomm, comm digests
LIST_FIELD = 5         # the opened list I
OPENED_FIELDS = (0, 1, 6, 7, 9, 10, 11, 12, 17, 18, 19, 20)
U16_FIELDS = tuple(f for f in range(24) if f not in BYTE_FIELDS and f != LIST_FIELD)
UNOPENED_FIELDS = tuple(f for f in U16_FIELDS if f not in OPENED_FIELDS)
LIMIT_BY_PARTY = {2: 407, 3: 407}
LIMIT_BY_INDEX = {8: 407, 15: 407, 16: 407, 21: 813, 22: 813}
LIMITED_FIELDS = tuple(sorted(set(LIMIT_BY_PARTY) | set(LIMIT_BY_INDEX)))
TAPE = 133  # the honest proof of the boundary set


def opened_list(p, pi):
    """(I, rest) of a proof image: field 5 as it stands and the unopened parties in ascending order"""
    I = [int(x) for x in np.frombuffer(pi, dtype="<u2", count=NOPEN, offset=p.off[LIST_FIELD])]
    opened = set(I)
    return I, [q for q in range(NPARTY) if q not in opened]


class ReadSet:
    def __init__(self, p, I, rest):
        assert len(I) == NOPEN and len(rest) == NREST and list(rest) == sorted(rest) and not set(I) & set(rest)
        self.p, self.I, self.rest = p, list(I), list(rest)
        self.records = {f: NOPEN if f in OPENED_FIELDS else NREST for f in U16_FIELDS}
        self.width = {f: p.size[f] // 2 // self.records[f] for f in U16_FIELDS}
        for f in U16_FIELDS:
            assert self.width[f] * self.records[f] * 2 == p.size[f], f

    def read(self, f, rec):
        assert 0 <= rec < self.records[f]
        if f in LIMIT_BY_PARTY:
            return self.rest[rec] < LIMIT_BY_PARTY[f]
        if f in LIMIT_BY_INDEX:
            return rec < LIMIT_BY_INDEX[f]
        return True

    def limit_records(self, f):
        """(last read record, first unread record) of a limited field"""
        n_read = sum(self.read(f, i) for i in range(NREST))
        assert 0 < n_read < NREST and all(self.read(f, i) == (i < n_read) for i in range(NREST))  # rest ascends: a prefix
        return n_read - 1, n_read

    def index(self, f, rec, elem):
        """u16 index inside field f of element elem (negative: from the record's end) of record rec"""
        w = self.width[f]
        return rec * w + (elem % w)

    def get(self, pi, f, idx):
        o = self.p.off[f] + 2 * idx
        return int.from_bytes(pi[o:o + 2], "little")

    def put(self, pi, f, idx, val):
        assert 0 <= val < 65536 and 0 <= idx < self.p.size[f] // 2
        t = bytearray(pi)
        o = self.p.off[f] + 2 * idx
        t[o:o + 2] = val.to_bytes(2, "little")
        return bytes(t)

    def strict_expectation(self, pi):
        """{field: number of u16 >= q in records the reference reads}, fields without one left out: the strict default rejects the
        image (fail bit 0) exactly when this is not empty"""
        out = {}
        for f in U16_FIELDS:
            a = np.frombuffer(pi, dtype="<u2", count=self.p.size[f] // 2, offset=self.p.off[f]).reshape(self.records[f], self.width[f])
            big = (a >= Q).sum(axis=1)
            n = sum(int(big[i]) for i in np.nonzero(big)[0] if self.read(f, int(i)))
            if n:
                out[f] = n
        return out


def boundary_records(m, f):
    """the records at which the read set of field f begins, ends and changes: (record, what)"""
    recs = [(0, "first"), (m.records[f] - 1, "last")]
    if f in LIMITED_FIELDS:
        lo, hi = m.limit_records(f)
        recs += [(lo, "last read"), (hi, "first unread")]
    return recs


def boundary_cases(m):
    """the first and the last element of every boundary record of every u16 field: [(field, record, element)], 112 of them"""
    return [(f, rec, elem) for f in U16_FIELDS for rec, _ in boundary_records(m, f) for elem in (0, m.width[f] - 1)]


def residue_image(m, pi, f, rec, elem):
    """pi with another canonical residue, (v + 1) % q, at that element: the image holds canonical elements only"""
    idx = m.index(f, rec, elem)
    return m.put(pi, f, idx, (m.get(pi, f, idx) + 1) % Q)


def oracle_verify_many(oracle, k, proofs, pk, threads=8):
    """the oracle's (bit, reason) on many proofs (tests/test_gpu_02_verify.py: _oracle_verify_many): tables by one call, then a
    small pool -- ctypes releases the interpreter lock"""
    from concurrent.futures import ThreadPoolExecutor
    first = oracle.kosk_verify(k, proofs[0], pk)
    with ThreadPoolExecutor(threads) as ex:
        return [first] + list(ex.map(lambda t: oracle.kosk_verify(k, t, pk), proofs[1:]))


@functools.lru_cache(maxsize=None)
def boundary_set(oracle, k):
    """(pk, pi, model, cases, oracle bits) of the honest oracle proof of tape 133: computed once per K and process, shared, never
    modified"""
    pk, _, pi, _, _ = oracle.verifiable_keygen(k, oracle.tape_bytes_for(k, TAPE))
    p = oracle.params(k)
    m = ReadSet(p, *opened_list(p, pi))
    cases = boundary_cases(m)
    bits = [ok for ok, _ in oracle_verify_many(oracle, k, [residue_image(m, pi, *c) for c in cases], pk)]
    return pk, pi, m, tuple(cases), tuple(bits)
