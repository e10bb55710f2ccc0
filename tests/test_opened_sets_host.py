"""CPU: the catalogue of opened lists (tests/opened_sets.py) reaches what it is there for, and the oracle's forcing prover
(ko_force_opened) makes proofs that fail the oracle's verifier at its last check only, and leaves no state behind."""
import pytest

from tests import opened_sets as osets


def test_catalogue_sets_are_well_formed():
    for name, I in osets.CATALOGUE.items():
        assert len(I) == 150 and len(set(I)) == 150 and min(I) >= 0 and max(I) < 1454, name
    assert sorted(osets.CATALOGUE["first150_shuffled"]) == osets.CATALOGUE["first150"]
    assert osets.CATALOGUE["first150_shuffled"] != osets.CATALOGUE["first150"]
    assert osets.CATALOGUE["first150_shuffled"] != sorted(osets.CATALOGUE["first150_shuffled"], reverse=True)


def test_catalogue_reaches_every_edge():
    sh = {name: osets.shape(I) for name, I in osets.CATALOGUE.items()}
    for name, s in sh.items():  # what holds for every list: the table indices stay inside the table, the three branches cover the points
        assert sum(s["points"].values()) == 407, name
        for t in s["sets"]:
            assert 0 <= t["idx_min"] <= t["idx_max"] < osets.TABLE_LEN, (name, t)
            assert t["hi"] - t["lo"] + 1 == (407 if t is s["sets"][0] else 813) + t["holes"], (name, t)
        assert s["max_hi_kp"] <= 556 + 256 and s["max_lo_kp"] <= 150 + 255, name

    for name in ("first150", "first150_shuffled"):
        s = sh[name]
        assert [t["lo"] for t in s["sets"]] == [150, 150] and [t["holes"] for t in s["sets"]] == [0, 0], s
        assert [t["hi"] for t in s["sets"]] == [556, 962], s
        # every evaluation point takes the below-lo branch, but the last: kp = 150 is lo itself, the first node
        assert s["points"] == {"below": 406, "hole": 0, "node": 1}, s
        assert s["max_lo_kp"] == 405 and s["max_hi_kp"] == 812, s      # the largest factorial indices of the below-lo branch
        assert s["first_windows_empty"] and s["empty_windows"] == 2, s
        assert s["sets"][0]["idx_max"] == 1709 and s["sets"][1]["idx_max"] == 1709 - 151, s  # no point above any node: 1/d for d <= 0 only

    s = sh["last150"]
    assert [(t["lo"], t["hi"], t["holes"]) for t in s["sets"]] == [(0, 406, 0), (0, 812, 0)], s
    assert s["points"] == {"below": 256, "hole": 0, "node": 151}, s
    assert s["last_windows_empty"] and s["empty_windows"] == 2, s

    s = sh["run100_249"]
    assert (s["sets"][0]["lo"], s["sets"][0]["hi"], s["sets"][0]["holes"]) == (0, osets.HI_MAX[0], 150), s
    assert s["points"] == {"below": 256, "hole": 51, "node": 100} and s["hole_run"] == 51, s
    assert s["sets"][1]["holes"] == 150 and s["sets"][1]["hi"] == osets.HI_MAX[1], s
    assert s["max_hi_kp"] == 812, s

    s = sh["above_points"]
    assert (s["sets"][0]["lo"], s["sets"][0]["hi"], s["sets"][0]["holes"]) == (0, osets.HI_MAX[0], 150), s
    assert s["points"] == {"below": 256, "hole": 0, "node": 151}, s     # every point k = 256..406 is a node
    assert min(osets.CATALOGUE["above_points"]) > 150                   # every hole above the points

    s = sh["mid600_749"]
    assert (s["sets"][0]["hi"], s["sets"][0]["holes"]) == (406, 0), s
    assert (s["sets"][1]["hi"], s["sets"][1]["holes"]) == (osets.HI_MAX[1], 150), s

    s = sh["every_third"]
    assert s["sets"][0]["lo"] == 1 and s["sets"][1]["lo"] == 1, s
    assert s["points"] == {"below": 257, "hole": 50, "node": 100} and s["hole_run"] == 1, s  # kp = 0 is opened AND below lo
    assert s["sets"][0]["holes"] == 149, s

    s = sh["spread"]
    assert {0, 63, 64, 1407, 1408, 1453} <= set(osets.CATALOGUE["spread"])
    assert s["sets"][0]["lo"] == 1 and s["empty_windows"] == 0, s
    # the extremes over the whole catalogue: the table's first and last entry that a live lane can load are both reached
    assert max(t["idx_max"] for s in sh.values() for t in s["sets"]) == 1709 + 150
    assert min(t["idx_min"] for s in sh.values() for t in s["sets"]) == 1709 - 256 - 981  # set 1 of first150: x_j = 256 + 150 + 831


def test_force_opened_rejects_bad_lists(oracle):
    good = list(range(150))
    try:
        assert oracle.force_opened(good[:-1] + [1454]) == -1
        assert oracle.force_opened(good[:-1] + [0xFFFF]) == -1
        assert oracle.force_opened(good[:-1] + [7]) == -1
        assert oracle.force_opened([3] + good[1:]) == -1
        assert oracle.force_opened(good[:-1] + [1453]) == 0
    finally:
        assert oracle.force_opened(None) == 0


def test_rejected_list_changes_nothing(oracle):
    """a list the hook rejects neither sets the hook nor overwrites the list that is set"""
    k = 2
    tape = oracle.tape_bytes_for(k, 211)
    plain = oracle.verifiable_keygen(k, tape)[:3]
    try:
        assert oracle.force_opened([5] * 150) == -1
        assert oracle.verifiable_keygen(k, tape)[:3] == plain
        I = osets.CATALOGUE["last150"]
        assert oracle.force_opened(I) == 0
        assert oracle.force_opened(I[:-1] + [I[0]]) == -1
        pi = oracle.verifiable_keygen(k, tape)[2]
    finally:
        oracle.force_opened(None)
    p = oracle.params(k)
    assert pi[p.off[5]:p.off[5] + 300] == b"".join(x.to_bytes(2, "little") for x in I)


@pytest.mark.parametrize("name", ["first150", "run100_249"])
def test_forced_proof_fails_the_last_check_only_and_the_hook_clears(name, oracle):
    k = 3
    p = oracle.params(k)
    I = osets.CATALOGUE[name]
    tape = oracle.tape_bytes_for(k, 210)
    plain = oracle.verifiable_keygen(k, tape)[:3]
    pk, sk, pi = oracle.forced_verifiable_keygen(k, tape, I)
    assert (pk, sk) == plain[:2]                                    # the key pair does not depend on the opened list
    assert pi[p.off[5]:p.off[5] + 300] == b"".join(x.to_bytes(2, "little") for x in I)   # in the given order
    ok, why = oracle.kosk_verify(k, pi, pk)
    assert not ok and why.startswith("Check failed for reom_I"), why
    # the hook is clear again: the same tape gives the plain proof, which verifies
    assert oracle.verifiable_keygen(k, tape)[:3] == plain
    assert oracle.kosk_verify(k, plain[2], plain[0])[0]
