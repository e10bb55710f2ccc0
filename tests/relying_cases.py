"""Case tables of the relying party's tests, shared by tests/test_relying_host.py and tests/test_gpu_39_relying.py and
built on registry_cases' fixture: 130 keys in 300 slots, D = 9.  A table is {"k", "depth", "root", "cases"}; a path case is (name, slot,
state, h, path, want), a proof case (name, x, record, want).  `want` is what the case was crafted for (None: whatever the host function
says); the EXPECTATION of every comparison is the host function's answer (host_paths / host_proofs), which test_relying_host.py holds
against the hashlib models (model_paths / model_proofs) and against `want`.  Built once per kyber_k, never modified."""
import ctypes as C
import functools
import hashlib
import random
import struct

from tests import kem_fixture as kf
from tests import registry_cases as rc
from tests import registry_sorted_model as sm
from tests import registry_tree_model as tm

D = tm.depth(rc.CAPACITY)
assert D == 9
INT32_MIN = -(1 << 31)
ZERO, ONES = bytes(32), b"\xff" * 32
MUTATIONS = 2000


def fp(tag):
    return hashlib.sha3_256(b"relying:" + tag).digest()


def flip(b, bit):
    b = bytearray(b)
    b[bit >> 3] ^= 1 << (bit & 7)
    return bytes(b)


@functools.lru_cache(maxsize=None)
def content(k):
    """{slot: SHA3-256(pk)} of the fixture registry"""
    return {rc.slot(i): hashlib.sha3_256(rc.pks(k)[i]).digest() for i in range(kf.ITEMS)}


@functools.lru_cache(maxsize=None)
def slot_levels(k):
    return tm.levels(k, rc.CAPACITY, content(k))


@functools.lru_cache(maxsize=None)
def sorted_levels(k):
    return sm.levels(k, rc.CAPACITY, content(k))


def empty_slots(k, count=10):
    return [s for s in range(rc.CAPACITY) if s not in content(k)][:count]


# ---- paths ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def path_table(k):
    """the fixture tree: every key, ten empty slots, and every way one field of a good item goes wrong"""
    c, lv = content(k), slot_levels(k)
    cases = [("key %d" % s, s, 1, c[s], tm.path(lv, s), 1) for s in sorted(c)]
    empties = empty_slots(k)
    cases += [("empty %d" % s, s, 0, fp(b"ignored"), tm.path(lv, s), 1) for s in empties]
    s0, e0 = rc.slot(0), empties[0]
    cases.append(("occupied claim on an empty slot", e0, 1, c[s0], tm.path(lv, e0), 0))
    cases.append(("empty claim on an occupied slot", s0, 0, c[s0], tm.path(lv, s0), 0))
    good = tm.path(lv, s0)
    for l in range(D):
        cases.append(("bit flipped at level %d" % l, s0, 1, c[s0], flip(good, 256 * l + 37 * l % 256), 0))
    cases.append(("bit flipped in h", s0, 1, flip(c[s0], 77), good, 0))
    for b in range(D):
        cases.append(("slot bit %d changed" % b, s0 ^ (1 << b), 1, c[s0], good, 0))
    for s in (-1, 1 << D, INT32_MIN):
        cases.append(("slot %d" % s, s, 1, c[s0], good, 0))
        cases.append(("slot %d claimed empty" % s, s, 0, c[s0], tm.path(lv, e0), 0))
    other = 2 + (k - 1) % 3  # another kyber_k: its tree over the same fingerprints
    cases.append(("a path made for kyber_k %d" % other, s0, 1, c[s0], tm.path(tm.levels(other, rc.CAPACITY, c), s0), 0))
    return {"k": k, "depth": D, "root": tm.root(lv), "cases": tuple(cases)}


@functools.lru_cache(maxsize=None)
def path_table_bad_root(k):
    """the good items of path_table under a root with one flipped bit: every item 0"""
    t = path_table(k)
    return {"k": k, "depth": D, "root": flip(t["root"], 200), "cases": tuple(c[:5] + (0,) for c in t["cases"] if c[5] == 1)}


@functools.lru_cache(maxsize=None)
def path_tables_depth_edges(k):
    """D = 0 (capacity 1, occupied and empty), D = 1, D = 11 (capacity 2 049, a key in slot 2 048)"""
    out = []
    h = fp(b"edge")
    for table in ({0: h}, {}):
        lv = tm.levels(k, 1, table)
        cases = [("D 0 occupied claim", 0, 1, h, b"", int(bool(table))), ("D 0 empty claim", 0, 0, h, b"", int(not table)),
                 ("D 0 slot 1", 1, 1, h, b"", 0), ("D 0 slot -1", -1, 0, h, b"", 0)]
        out.append({"k": k, "depth": 0, "root": tm.root(lv), "cases": tuple(cases)})
    lv = tm.levels(k, 2, {1: h})
    cases = [("D 1 key", 1, 1, h, tm.path(lv, 1), 1), ("D 1 empty", 0, 0, h, tm.path(lv, 0), 1), ("D 1 key on the other side", 0, 1, h, tm.path(lv, 1), 0),
             ("D 1 slot 2", 2, 1, h, tm.path(lv, 1), 0)]
    out.append({"k": k, "depth": 1, "root": tm.root(lv), "cases": tuple(cases)})
    table = {2048: h, 5: fp(b"edge5")}
    slv, blank = tm.sparse_root(k, 2049, table)
    d = tm.depth(2049)
    assert d == 12  # 2 049 slots need 2^12 leaves; the issue's "D = 11" names the capacity 2^11 + 1
    cases = [("slot 2048", 2048, 1, h, tm.sparse_path(slv, blank, 2048), 1), ("slot 5", 5, 1, table[5], tm.sparse_path(slv, blank, 5), 1),
             ("empty 2049", 2049, 0, h, tm.sparse_path(slv, blank, 2049), 1), ("empty 4095", 4095, 0, h, tm.sparse_path(slv, blank, 4095), 1),
             ("slot 4096", 4096, 0, h, tm.sparse_path(slv, blank, 4095), 0), ("slot 2048 with the path of 5", 2048, 1, h, tm.sparse_path(slv, blank, 5), 0)]
    out.append({"k": k, "depth": d, "root": slv[d][0], "cases": tuple(cases)})
    # D = 11 itself: capacity 2 048, keys in the last slot and in slot 1 024
    table = {2047: h, 1024: fp(b"edge1024")}
    slv, blank = tm.sparse_root(k, 2048, table)
    cases = [("slot 2047", 2047, 1, h, tm.sparse_path(slv, blank, 2047), 1), ("slot 1024", 1024, 1, table[1024], tm.sparse_path(slv, blank, 1024), 1),
             ("slot 2048", 2048, 1, h, tm.sparse_path(slv, blank, 2047), 0), ("empty 0", 0, 0, h, tm.sparse_path(slv, blank, 0), 1)]
    out.append({"k": k, "depth": 11, "root": slv[11][0], "cases": tuple(cases)})
    return tuple(out)


def path_table_depth31(api, k):
    """D = 31, synthetic: 31 siblings from a fixed seed per slot, the root from the host function.  One table per slot (a call has one root)"""
    out = []
    rnd = random.Random(3100 + k)
    h = fp(b"deep")
    for slot in (0, 1 << 30, (1 << 31) - 1):
        path = bytes(rnd.getrandbits(8) for _ in range(31 * 32))
        root = api.regtree_root_from_path(k, 31, slot, h, path)
        cases = [("D 31 slot %d" % slot, slot, 1, h, path, 1), ("D 31 slot %d, bit 30 changed" % slot, slot ^ (1 << 30), 1, h, path, 0),
                 ("D 31 slot %d, top level flipped" % slot, slot, 1, h, flip(path, 256 * 30 + 5), 0), ("D 31 INT32_MIN", INT32_MIN, 1, h, path, 0),
                 ("D 31 slot -1", -1, 1, h, path, 0)]
        out.append({"k": k, "depth": 31, "root": root, "cases": tuple(cases)})
    return out


def all_path_tables(api, k):
    return [path_table(k), path_table_bad_root(k)] + list(path_tables_depth_edges(k)) + path_table_depth31(api, k)


def host_paths(api, t):
    """the host function on every case: 1 iff it returns 0 and its root is the table's"""
    out = []
    got = C.create_string_buffer(32)
    for _name, slot, state, h, path, _want in t["cases"]:
        r = api.lib.kosk_regtree_root_from_path(t["k"], t["depth"], slot, C.c_char_p(h) if state else None, C.c_char_p(path) if t["depth"] else None, got)
        out.append(1 if r == 0 and got.raw == t["root"] else 0)
    return out


def model_paths(t):
    d = t["depth"]
    return [1 if 0 <= slot < (1 << d) and tm.root_from_path(t["k"], d, slot, h if state else None, path) == t["root"] else 0
            for _name, slot, state, h, path, _want in t["cases"]]


def path_args(t):
    """(slots, hs, paths, states) of a table, as Kosk.regtree_check_paths takes them"""
    cases = t["cases"]
    return [c[1] for c in cases], [c[3] for c in cases], ([c[4] for c in cases] if t["depth"] else None), [c[2] for c in cases]


# ---- proofs --------------------------------------------------------------------------------------------------------------
def _parts(rec, d):
    pos_l, slot_l, slot_r, flags = struct.unpack("<iiiI", rec[:16])
    return [pos_l, slot_l, slot_r, flags, rec[16:48], rec[48:80], rec[80:80 + 32 * d], rec[80 + 32 * d:]]


def _edit(rec, d, **kw):
    names = ["pos_l", "slot_l", "slot_r", "flags", "h_l", "h_r", "path_l", "path_r"]
    p = _parts(rec, d)
    for name, v in kw.items():
        p[names.index(name)] = v
    return sm.record(*p)


@functools.lru_cache(maxsize=None)
def proof_table(k):
    """the fixture's sorted tree: the valid records, one record per `return` of regsort::check_proof (named R1..R8 in source order; the
    `return -1` in front of them is the refusal of bad arguments, which no record reaches), and 2 000 single-byte mutations"""
    c, lv = content(k), sorted_levels(k)
    root, ent, P = sm.root(lv), sm.entries(content(k)), 1 << D

    def prove(x):
        return sm.prove(k, rc.CAPACITY, c, x, lv)
    cases = []
    between = []
    for i in (0, 1, 2, 64, 65, 127, 128, 129):
        between += sm.neighbours(ent[i][0])
    for x in between:
        kind, rec = prove(x)
        assert kind == sm.ABSENT
        cases.append(("ABSENT next to a key", x, rec, sm.ABSENT))
    assert any(_parts(cs[2], D)[3] == 7 for cs in cases)  # both neighbours
    assert ent[0][0] != ZERO and ent[-1][0] != ONES
    cases.append(("ABSENT without a left neighbour", ZERO, prove(ZERO)[1], sm.ABSENT))
    assert _parts(cases[-1][2], D)[:4] == [-1, 0, ent[0][1], 6]
    cases.append(("ABSENT, the right neighbour is Z", ONES, prove(ONES)[1], sm.ABSENT))
    assert _parts(cases[-1][2], D)[:4] == [len(ent) - 1, ent[-1][1], 0, 3]
    for h, _s in ent:
        cases.append(("PRESENT", h, prove(h)[1], sm.PRESENT))
    # one record per return statement, from a both-neighbours record `mid`, a PRESENT record `here` and the two edge records
    x = sm.neighbours(ent[64][0])[1]
    mid = prove(x)[1]
    assert _parts(mid, D)[3] == 7 and _parts(mid, D)[0] == 64
    xh = ent[64][0]
    here = prove(xh)[1]
    crafted = [
        ("R1 PRESENT holds", xh, here, sm.PRESENT),
        ("R1 PRESENT: h_l is not x", x, here, sm.NEITHER),
        ("R1 PRESENT: pos_l = -1", xh, _edit(here, D, pos_l=-1), sm.NEITHER),
        ("R1 PRESENT: pos_l = P", xh, _edit(here, D, pos_l=P), sm.NEITHER),
        ("R1 PRESENT: the walk fails", xh, _edit(here, D, path_l=flip(_parts(here, D)[6], 700)), sm.NEITHER),
        ("R1 PRESENT: slot_l < 0", xh, _edit(here, D, slot_l=-5), sm.NEITHER),
        ("R2 a flag above bit 2", x, _edit(mid, D, flags=7 | 16), sm.NEITHER),
        ("R2 bit 3 with a right record", x, _edit(mid, D, flags=15), sm.NEITHER),
        ("R2 neither side", x, _edit(mid, D, flags=0), sm.NEITHER),
        ("R2 a right key without a right record", x, _edit(mid, D, flags=5), sm.NEITHER),
        ("R3 left: pos_l < 0", x, _edit(mid, D, pos_l=-1), sm.NEITHER),
        ("R3 left: pos_l = P", x, _edit(mid, D, pos_l=P), sm.NEITHER),
        ("R3 left: h_l equals x", xh, mid, sm.NEITHER),
        ("R3 left: h_l above x", sm.neighbours(xh)[0], mid, sm.NEITHER),
        ("R3 left: the walk fails", x, _edit(mid, D, path_l=flip(_parts(mid, D)[6], 1)), sm.NEITHER),
        ("R3 left: slot_l < 0", x, _edit(mid, D, slot_l=INT32_MIN), sm.NEITHER),
        ("R4 no left record but pos_l = 0", ZERO, _edit(prove(ZERO)[1], D, pos_l=0), sm.NEITHER),
        ("R6 right key: x equals h_r", ent[65][0], _edit(mid, D), sm.NEITHER),
        ("R6 right key: x above h_r", sm.neighbours(ent[65][0])[1], mid, sm.NEITHER),
        ("R6 right key: the walk fails", x, _edit(mid, D, path_r=flip(_parts(mid, D)[7], 32 * 8 * 8 + 3)), sm.NEITHER),
        ("R6 right key: slot_r < 0", x, _edit(mid, D, slot_r=-1), sm.NEITHER),
        ("R6 right Z: the walk fails", ONES, _edit(prove(ONES)[1], D, path_r=flip(_parts(prove(ONES)[1], D)[7], 9)), sm.NEITHER),
        ("R6 right Z claimed where a key stands", x, _edit(mid, D, flags=3), sm.NEITHER),
        ("R7 no right record but pos_l is not P - 1", x, _edit(mid, D, flags=1), sm.NEITHER),
        ("R8 ABSENT", x, mid, sm.ABSENT),
    ]
    cases += crafted
    # 2 000 single-byte mutations of valid records: whatever the host function says of them
    pool = [(cs[1], cs[2]) for cs in cases if cs[0].startswith(("ABSENT", "PRESENT"))]
    rnd = random.Random(20390 + k)
    for i in range(MUTATIONS):
        qx, rec = pool[rnd.randrange(len(pool))]
        at, v = rnd.randrange(len(rec)), rnd.randrange(1, 256)
        bad = bytearray(rec)
        bad[at] ^= v
        cases.append(("mutation %d: byte %d ^ %02x" % (i, at, v), qx, bytes(bad), None))
    return {"k": k, "depth": D, "root": root, "cases": tuple(cases)}


@functools.lru_cache(maxsize=None)
def proof_table_full(k):
    """capacity 8 holding 8 keys: ABSENT records in a full table, among them a query above all keys (no right record, pos_l = P - 1), and the
    returns only a full table reaches (R5, R7 with a right edge)"""
    c = {s: fp(b"full:%d" % s) for s in range(8)}
    lv = sm.levels(k, 8, c)
    ent, d = sm.entries(c), 3
    cases = []
    for x in [ZERO, ONES] + [q for h, _s in ent for q in sm.neighbours(h)]:
        kind, rec = sm.prove(k, 8, c, x, lv)
        assert kind == sm.ABSENT
        cases.append(("full table: ABSENT", x, rec, sm.ABSENT))
    top = sm.prove(k, 8, c, ONES, lv)[1]
    assert _parts(top, d)[:4] == [7, ent[-1][1], 0, 1]
    cases.append(("R5 a right record behind the last position", ONES, _edit(top, d, flags=3), sm.NEITHER))
    cases.append(("R5 a right key behind the last position", ONES, _edit(top, d, flags=7), sm.NEITHER))
    low = sm.prove(k, 8, c, sm.neighbours(ent[3][0])[1], lv)[1]
    cases.append(("R7 no right record at position 3", sm.neighbours(ent[3][0])[1], _edit(low, d, flags=1), sm.NEITHER))
    for h, _s in ent:
        cases.append(("full table: PRESENT", h, sm.prove(k, 8, c, h, lv)[1], sm.PRESENT))
    return {"k": k, "depth": d, "root": sm.root(lv), "cases": tuple(cases)}


def all_proof_tables(k):
    return [proof_table(k), proof_table_full(k)]


def host_proofs(api, t):
    return [api.regsort_check_proof(t["k"], t["depth"], x, rec, t["root"]) for _name, x, rec, _want in t["cases"]]


def model_proofs(t):
    return [sm.check(t["k"], t["depth"], x, rec, t["root"]) for _name, x, rec, _want in t["cases"]]
