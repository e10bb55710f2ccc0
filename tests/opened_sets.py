"""Opened lists I at the edges of the verifier's interpolation set-up, with a plain-Python model of what each one reaches.  Tests
only; it calls nothing of the library.

The verifier's per-proof arithmetic is keyed by I (150 of 1454 parties) and its ascending complement `rest`: the nodes of the
degree-d interpolation are the parties rest[0..406] ("set 0"), those of the degree-2d interpolation rest[0..812] ("set 1"); lo = rest[0],
hi = rest[406] or rest[812]; the opened parties inside [lo, hi] are the holes of the barycentric weights.  A list out of the
Fiat-Shamir hash has lo in {0, 1}, hi near 450 / 905, about 47 / 94 holes and no empty 64-party window: the sets below are what such a
list never is.  shape(I) says, from the definitions alone, which branches and table indices a list reaches."""
import random

NPARTY, NOPEN, NSEC, DEG, DEG2 = 1454, 150, 256, 406, 812
NREST = NPARTY - NOPEN
LOADED = (448, 832)   # nodes per set that the product walks (7 and 13 k-steps of 64): more than the 407 / 813 that carry a weight
TABLE_OFF = NPARTY - 1 + NSEC                  # 1709: the inverse of d sits at table index d + 1709
TABLE_LEN = TABLE_OFF + (DEG - NSEC) + 1       # 1860 entries: d in [-1709, 150]


def complement(I):
    opened = set(int(p) for p in I)
    assert len(opened) == NOPEN == len(I) and all(0 <= p < NPARTY for p in opened)
    return [p for p in range(NPARTY) if p not in opened]


def shape(I):
    """What the opened list I reaches in the verifier's set-up and interpolation kernels:
    sets[s] for s = 0 (407 nodes) and 1 (813 nodes): lo, hi, holes = opened parties inside [lo, hi], idx_min / idx_max = the
        smallest / largest table index k - x_j + 1709 over the evaluation points k (0..406, or 0..255 for set 1) and the loaded
        nodes x_j = 256 + rest[j], j < 448 / 832;
    points: for set 0, how many of the evaluation points kp = -256..150 (k = kp + 256) lie below lo, on a hole, on a node;
    hole_run: the longest run of consecutive evaluation points that are holes;
    max_hi_kp, max_lo_kp: the largest hi - kp and lo - 1 - kp (factorial-table indices of the below-lo branch; hi - kp also of the
        hole branch);
    empty_windows: aligned 64-party windows [64 w, 64 w + 64) that hold no unopened party."""
    rest = complement(I)
    opened = set(int(p) for p in I)
    sets = []
    for s, n in enumerate((DEG + 1, DEG2 + 1)):
        lo, hi = rest[0], rest[n - 1]
        neval = DEG + 1 if s == 0 else NSEC
        idx = [k - (NSEC + rest[j]) + TABLE_OFF for k in (0, neval - 1) for j in (0, LOADED[s] - 1)]   # monotone in k and in j
        sets.append({"lo": lo, "hi": hi, "holes": sum(lo <= p <= hi for p in opened), "idx_min": min(idx), "idx_max": max(idx)})
    lo, hi = sets[0]["lo"], sets[0]["hi"]
    points = {"below": 0, "hole": 0, "node": 0}
    run = hole_run = 0
    for kp in range(-NSEC, DEG - NSEC + 1):
        kind = "below" if kp < lo else "hole" if kp in opened else "node"
        points[kind] += 1
        run = run + 1 if kind == "hole" else 0
        hole_run = max(hole_run, run)
    windows = [sum(p not in opened for p in range(w, min(w + 64, NPARTY))) for w in range(0, NPARTY, 64)]
    return {"sets": sets, "points": points, "hole_run": hole_run, "max_hi_kp": hi + NSEC, "max_lo_kp": lo - 1 + NSEC,
            "empty_windows": sum(c == 0 for c in windows), "first_windows_empty": windows[0] == 0 and windows[1] == 0,
            "last_windows_empty": windows[-1] == 0 and windows[-2] == 0}


def _shuffled(seq, seed):
    out = list(seq)
    random.Random(seed).shuffle(out)
    return out


SPREAD = [0, 63, 64, 1407, 1408, 1453] + list(range(5, 1445, 10))

# name -> I, in the order the proof holds it
CATALOGUE = {
    "first150": list(range(150)),                    # lo = 150: 406 points below lo, the last one on lo; no holes; windows 0 and 1 empty
    "first150_shuffled": _shuffled(range(150), 21),  # the same set: the order of I is the order of the opened records
    "last150": list(range(1304, 1454)),              # hi = 406 / 812 (their minimum), no holes, the last two windows empty
    "run100_249": list(range(100, 250)),             # 51 consecutive hole points, 100 node points, hi = 556 (set 0's maximum), 150 holes
    "above_points": list(range(257, 407)),           # hi = 556, every point 256..406 a node, every hole above the points
    "mid600_749": list(range(600, 750)),             # set 0 without holes, set 1 with 150 holes and hi = 962 (its maximum)
    "every_third": list(range(0, 450, 3)),           # holes and nodes alternating, party 0 opened, lo = 1
    "spread": SPREAD,                                # window edges, first and last party opened
}

HI_MAX = (DEG + NOPEN, DEG2 + NOPEN)  # 556, 962: every opened party below the last node


# ---- the prover's side: from 150 candidates to the list I and the tables the wire-image kernel reads (kosk_params.hpp)
NWIN = (NPARTY + 63) // 64                                # 23 aligned windows of 64 parties, the last one 46 wide
SEL_WIN, SEL_OSORT, SEL_OPOS = 160, 192, 352              # where a row of the opened-list table holds win, osort, opos behind I
SEL_ENTRIES = SEL_OPOS + NOPEN                            # 502 documented entries of a sel row; a rest row has NREST


def probe(cand):
    """The opened list of the candidates: entry i is (cand[i] + inc) % 1454 for the smallest inc >= 0 at which that party is not
    among the entries before it."""
    assert len(cand) == NOPEN and all(0 <= int(c) < NPARTY for c in cand)
    I, taken = [], set()
    for c in cand:
        inc = 0
        while (int(c) + inc) % NPARTY in taken:
            inc += 1
        I.append((int(c) + inc) % NPARTY)
        taken.add(I[-1])
    return I


def chain_shape(cand):
    """(longest, total, wrapped): the largest inc of an entry, the sum of all inc, and how many entries went past party 1453 to get
    to their place."""
    I = probe(cand)
    inc = [(p - int(c)) % NPARTY for p, c in zip(I, cand)]
    return max(inc), sum(inc), sum(int(c) + d >= NPARTY for c, d in zip(cand, inc))


def tables(I):
    """(rest, win, osort, opos) of the list I: the ascending complement (1304 parties); win[w], w = 0..23: how many unopened parties
    lie below party 64 w; the opened parties ascending; and the position in I of each of those."""
    rest = complement(I)
    where = {int(p): i for i, p in enumerate(I)}
    win = [sum(p < 64 * w for p in rest) for w in range(NWIN + 1)]
    osort = sorted(where)
    return rest, win, osort, [where[p] for p in osort]


def windows(I):
    """opened parties in each of the 23 aligned 64-party windows (nk of the wire-image kernel; cnt = the window's width - nk)"""
    opened = set(int(p) for p in I)
    return [sum(p in opened for p in range(w, min(w + 64, NPARTY))) for w in range(0, NPARTY, 64)]


def sel_row(I):
    """the documented entries of a sel row as {index: value}"""
    _, win, osort, opos = tables(I)
    row = {i: int(p) for i, p in enumerate(I)}
    row.update({SEL_WIN + w: v for w, v in enumerate(win)})
    row.update({SEL_OSORT + k: v for k, v in enumerate(osort)})
    row.update({SEL_OPOS + k: v for k, v in enumerate(opos)})
    return row


# name -> 150 candidates; duplicates are what reaches the probing.  probe(CANDIDATES[name]) is the list the prover opens
CANDIDATES = {
    "all_1453": [1453] * 150,                                      # I = 1453, 0, 1, .., 148: entry i probes i steps, all but the first wrap
    "zigzag": [0, 1453] * 75,                                      # I = 0, 1453, 1, 2, .., 148: chains from both ends of the party range
    "top_then_1400": list(range(1354, 1454)) + [1400] * 50,        # 50 chains through the filled top 1400..1453 and over the wrap to 0..49
    "tail_chain": list(range(500, 649)) + [500],                   # one chain of 149 steps in the middle, no wrap: I = 500..649
    "pairs": [v for v in range(7, 7 + 19 * 75, 19) for _ in (0, 1)],  # 75 chains of one step; opened parties in every window
}
