"""The prover at forced opened lists, the part that needs no GPU: the model of tests/opened_sets.py (probe, tables, chain_shape,
windows) against a brute-force restatement; the shapes that the catalogue is there for, pinned, so that a case which no longer reaches
its edge fails here; the host's round-2 function behind the PRF (kosk_opened_tables: opened_from_candidates + opened_derived_tables of
kosk_host.cpp, what fs_opened_batch runs per proof) against the model, whole rows; the oracle's forcing prover accepts every list."""
import ctypes as C
import os
import random

import pytest

from tests import opened_sets as osets

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, T = osets.NPARTY, osets.NOPEN
FILL = 0xA5A5  # what a row holds before the call: no party, no position, no count


@pytest.fixture(scope="module")
def api():
    from mpcith_kyber_kosk_amd import api
    return api


def all_cases():
    """name -> candidates: every CATALOGUE list given as its own candidates (distinct: the list comes back), every CANDIDATES case"""
    cases = dict(osets.CATALOGUE)
    cases.update(osets.CANDIDATES)
    return cases


def random_candidates(count, seed):
    """candidate lists with few, some and many duplicates, near the wrap and away from it"""
    rng = random.Random(seed)
    out = []
    for i in range(count):
        kind = i % 5
        if kind == 0:
            out.append([rng.randrange(N) for _ in range(T)])                      # as out of the hash: a few chains of a few steps
        elif kind == 1:
            base, span = rng.randrange(N), rng.randrange(1, 40)
            out.append([(base + rng.randrange(span)) % N for _ in range(T)])      # 150 candidates in a span below 40: long chains, maybe over the wrap
        elif kind == 2:
            out.append([N - 1 - rng.randrange(rng.randrange(1, 200)) for _ in range(T)])  # the top of the range: wraps
        elif kind == 3:
            pool = [rng.randrange(N) for _ in range(rng.randrange(1, 30))]
            out.append([rng.choice(pool) for _ in range(T)])                      # a few values, many times each
        else:
            lst = rng.sample(range(N), T)
            out.append(lst[:75] + lst[:75])                                       # every value twice, the second time far behind the first
    return out


def brute_probe(cand):
    """entry i from the definition alone: try inc = 0, 1, 2, ... and look through all entries before i every time"""
    I = []
    for c in cand:
        I.append(next((c + inc) % N for inc in range(N) if all((c + inc) % N != p for p in I)))
    return I


def expected_rows(I, stride, fill=FILL):
    sel, rest = [fill] * stride, [fill] * stride
    for i, v in osets.sel_row(I).items():
        sel[i] = v
    rest[:osets.NREST] = osets.tables(I)[0]
    return sel, rest


# ---- the model
def test_probe_is_the_definition_on_random_lists():
    for cand in random_candidates(60, 1) + list(all_cases().values()):
        I = osets.probe(cand)
        assert I == brute_probe(cand)
        assert len(set(I)) == T


def test_tables_follow_their_definitions():
    for cand in random_candidates(20, 2) + list(all_cases().values()):
        I = osets.probe(cand)
        rest, win, osort, opos = osets.tables(I)
        assert sorted(rest + list(I)) == list(range(N)) and rest == sorted(rest) and len(rest) == osets.NREST
        assert len(win) == osets.NWIN + 1 == 24 and win[0] == 0 and win[-1] == osets.NREST
        nk = osets.windows(I)
        for w in range(osets.NWIN):
            width = min(64, N - 64 * w)
            assert win[w + 1] - win[w] == width - nk[w]              # cnt of window w
            assert rest[win[w]:win[w + 1]] == [p for p in range(64 * w, 64 * w + width) if p not in set(I)]
        assert osort == sorted(I) and [I[i] for i in opos] == osort


def test_the_catalogue_lists_are_their_own_candidates():
    for name, I in osets.CATALOGUE.items():
        assert osets.probe(I) == list(I), name
        assert osets.chain_shape(I) == (0, 0, 0), name


# ---- what each case is there for
def test_candidate_cases_have_the_shapes_they_are_there_for():
    c = osets.CANDIDATES
    assert osets.probe(c["all_1453"]) == [1453] + list(range(149))
    assert osets.chain_shape(c["all_1453"]) == (149, 11175, 149)
    assert osets.probe(c["zigzag"]) == [0, 1453] + list(range(1, 149))
    longest, _, wrapped = osets.chain_shape(c["zigzag"])
    assert (longest, wrapped) == (149, 74)
    I = osets.probe(c["top_then_1400"])
    assert I == list(range(1354, 1454)) + list(range(50))
    longest, _, wrapped = osets.chain_shape(c["top_then_1400"])
    assert (longest, wrapped) == (103, 50)
    assert osets.probe(c["tail_chain"]) == list(range(500, 650))
    assert osets.chain_shape(c["tail_chain"]) == (149, 149, 0)
    I = osets.probe(c["pairs"])
    assert I == [v + d for v in range(7, 7 + 19 * 75, 19) for d in (0, 1)]
    assert osets.chain_shape(c["pairs"]) == (1, 75, 0)
    assert min(osets.windows(I)) >= 1                                    # no window without an opened party
    # a list out of the hash (2 000 modelled): chains of at most 7 steps, at most 18 opened parties per window
    assert all(osets.chain_shape(x)[0] >= 100 for x in (c["all_1453"], c["zigzag"], c["top_then_1400"], c["tail_chain"]))


def test_window_counts_reach_the_edges_of_the_image_kernel():
    lists = {name: osets.probe(c) for name, c in all_cases().items()}
    nk = {name: osets.windows(I) for name, I in lists.items()}
    assert nk["first150"][:3] == [64, 64, 22] and nk["first150_shuffled"] == nk["first150"]
    assert nk["last150"][-3:] == [40, 64, 46]                            # the short last window entirely opened
    assert nk["above_points"][4:7] == [63, 64, 23]
    assert set(nk["every_third"][:7]) == {21, 22}
    assert nk["top_then_1400"][-2:] == [54, 46] and nk["top_then_1400"][0] == 50
    assert nk["all_1453"][:3] == [64, 64, 21] and nk["all_1453"][-1] == 1
    spread = set(lists["spread"])
    assert {0, 63, 64, 1407, 1408, 1453} <= spread                       # opened parties at both edges of windows
    # opened kind: nk = 0 in a run of 20 windows and more, nk = 64, every row of the 64 x 80 tile; nk = 46 = the whole last window
    run = best = 0
    for v in nk["first150"]:
        run = run + 1 if v == 0 else 0
        best = max(best, run)
    assert best == 20
    reached = set(v for w in nk.values() for v in w)
    assert {0, 1, 2, 63, 64} <= reached and max(reached) == 64
    assert sum(w[-1] == 46 for w in nk.values()) >= 2
    # unopened kind: cnt = 64 (nothing opened), cnt = 0 (the early return) in full windows and in the last one
    cnt = set(min(64, N - 64 * w) - v for x in nk.values() for w, v in enumerate(x))
    assert {0, 1, 64} <= cnt and nk["last150"][-1] == N - 64 * (osets.NWIN - 1)
    # i0 = win[w] of windows that hold unopened parties: both parities, so i0 * width does for every field width (odd and even)
    for name in ("spread", "pairs", "every_third"):
        win = osets.tables(lists[name])[1]
        assert {win[w] & 1 for w in range(osets.NWIN) if win[w + 1] > win[w]} == {0, 1}, name


# ---- the host's function against the model
def test_opened_tables_whole_rows(api):
    cases = list(all_cases().items()) + [("random%d" % i, c) for i, c in enumerate(random_candidates(200, 3))]
    assert len(cases) == 213
    for name, cand in cases:
        I = osets.probe(cand)
        stride = 1304 if name == "last150" else 1312 if name != "zigzag" else 1500
        sel, rest = api.opened_tables(cand, sel_stride=stride, fill=FILL)
        esel, erest = expected_rows(I, stride)
        if sel != esel or rest != erest:
            row, got, exp = ("sel", sel, esel) if sel != esel else ("rest", rest, erest)
            at = next(i for i in range(stride) if got[i] != exp[i])
            pytest.fail("%s: %s row differs at entry %d: %d, expected %d (candidates %r)" % (name, row, at, got[at], exp[at], cand))


def test_opened_tables_argument_errors(api):
    lib = api.lib
    ok = (C.c_uint16 * 150)(*range(150))
    sel, rest = (C.c_uint16 * 1312)(), (C.c_uint16 * 1312)()
    assert lib.kosk_opened_tables(ok, sel, rest, 1312) == 0
    assert lib.kosk_opened_tables(ok, sel, rest, 1304) == 0
    before = (list(sel), list(rest))
    assert lib.kosk_opened_tables(ok, sel, rest, 1303) == -1
    assert lib.kosk_opened_tables(None, sel, rest, 1312) == -1
    assert lib.kosk_opened_tables(ok, None, rest, 1312) == -1
    assert lib.kosk_opened_tables(ok, sel, None, 1312) == -1
    for at in (0, 77, 149):
        bad = (C.c_uint16 * 150)(*range(150))
        bad[at] = 1454
        assert lib.kosk_opened_tables(bad, sel, rest, 1312) == -1
        bad[at] = 65535
        assert lib.kosk_opened_tables(bad, sel, rest, 1312) == -1
    assert (list(sel), list(rest)) == before                             # a refused call writes nothing
    with pytest.raises(api.KoskError):
        api.opened_tables([1454] * 150)
    with pytest.raises(api.KoskError):
        api.opened_tables(list(range(149)))
    assert lib.kosk_force_opened_candidates(None, 1, ok) == -1          # no handle


def test_abi(api):
    hdr = open(os.path.join(ROOT, "include", "kosk_mi355x.h")).read()
    for name in ("kosk_force_opened_candidates", "kosk_opened_tables"):
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib, name), name


# ---- the oracle's forcing prover takes every list
def test_oracle_accepts_every_probed_list(oracle):
    try:
        for name, cand in all_cases().items():
            assert oracle.force_opened(osets.probe(cand)) == 0, name
        assert oracle.force_opened(osets.CANDIDATES["all_1453"]) == -1    # candidates with duplicates are not a list
    finally:
        oracle.force_opened(None)
