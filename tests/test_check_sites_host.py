"""CPU: every case of tests/check_sites.py breaks exactly the check(s) it is meant to break, at one site where the catalogue gives a
count, and no hash -- proven on the oracle alone, by its verifier that goes on after a failed comparison (ko_kosk_verify_sites).  The
GPU's fail masks are compared with these in tests/test_gpu_23_check_sites.py."""
import pytest

from tests import check_sites as cs

MANY = 64  # "many sites": one moved secret of beta moves every NTT output it reaches, a wrong u row every reconstructed secret
# what ko_kosk_verify says when a check fails -> its fail bit
REASON_BIT = (("malformed opened-party list", 0), ("beta[", 1), ("s + r share error", 2), ("e + r share error", 2), ("for NTT(s[", 3),
              ("for NTT(e[", 3), ("NTT(A*(s[", 4), ("Check failed for t[", 5), ("t = A*s + e", 6), ("_eta[", 7), ("s - eta at view", 8),
              ("e - eta at view", 8), (".u[", 9), ("u2d[", 10), ("reom_I", 11))


def reason_bit(why):
    hits = {bit for text, bit in REASON_BIT if text in why}
    assert len(hits) == 1, why
    return hits.pop()


def test_catalogue_is_at_the_edges():
    """the corners the catalogue promises, per K, from the names alone"""
    for k in (2, 3, 4):
        names = cs.names(k)
        rows = {n.split(":")[0] for n in names}
        assert rows == set(cs.ROWS), k
        assert len(names) == (sum(len(r[3]) for r in cs.ROWS.values()) if k == 3 else 2 * len(cs.ROWS))
        text = " ".join(names)
        for need in ("i=0", "i=L", "c=0", "c=255", "j=0", "j=149", "side=s", "side=e", "m=0", "m=L", "z=0", "z=L", "col=0", "col=69",
                     "pos=407", "pos=1303"):
            assert need in text, (k, need)
    all3 = " ".join(cs.names(3))
    for need in ("pos=1279", "pos=1280", "c=63", "c=64", "j=64"):
        assert need in all3, need
    for row in ("sub_eta", "eta"):  # K = 2: gate m = 6, the last slot of MAXE = 7; K = 4: polynomial i = 3, the last slot of MAXK = 4
        assert any(n.startswith(row + ":") and "i=L" in n and "m=L" in n for n in cs.names(2)), row
    for row in ("t_pk", "t_pk_pkside", "sr_er", "ntt_e", "sub_eta"):
        assert any(n.startswith(row + ":") and "i=L" in n for n in cs.names(4)), row
    assert set(cs.CATALOGUE) == set(cs.names(3))
    bits = set()
    for b, _ in cs.CATALOGUE.values():
        bits |= set(b)
    assert bits == set(range(1, 11))


@pytest.fixture(scope="module", params=[2, 3, 4])
def built(request, oracle):
    """(k, the honest proof and every case of this K, the counting oracle's (mask, sites) per case name)"""
    k = request.param
    b = cs.build(oracle, k)
    names = list(b["cases"])
    exp = cs.expected(oracle, k, [(b["cases"][n][1], b["cases"][n][0]) for n in names])
    return k, b, dict(zip(names, exp))


def test_honest_proof_has_no_failing_site(built, oracle):
    k, b, _ = built
    pk, pi = b["honest"]
    assert oracle.kosk_verify_sites(k, pi, pk) == (True, [0] * 12)
    assert oracle.kosk_verify(k, pi, pk) == (True, "")
    assert cs.opened_and_rest(k, pi)[0] != sorted(cs.opened_and_rest(k, pi)[0])  # positions in I are not parties in order


def test_every_case_breaks_its_checks_only(built, oracle):
    """no case is left out: one that does not behave as the catalogue says fails this test"""
    k, b, exp = built
    p = oracle.params(k)
    assert (p.E, p.Z) == {2: (7, 6), 3: (5, 4), 4: (5, 4)}[k]
    bad = []
    for name in cs.names(k):
        bits, count = cs.CATALOGUE[name]
        mask, sites = exp[name]
        pk, pi = b["cases"][name]
        assert (pi == b["honest"][1]) == cs.is_pk_case(name) and (pk == b["honest"][0]) != cs.is_pk_case(name), name
        ok = mask == cs.intended_mask(name) and not mask & (1 | 1 << 11)
        for n, bit in enumerate(bits):
            ok = ok and (sites[bit] == count[n] if count is not None else sites[bit] >= MANY)
        if not ok:
            bad.append((name, hex(mask), sites))
    assert not bad, "k=%d: %r" % (k, bad)


def test_first_failure_verifier_names_the_lowest_bit(built, oracle):
    """ko_kosk_verify (first failure, then stop) rejects every case, for the reason of its lowest intended bit"""
    from concurrent.futures import ThreadPoolExecutor
    k, b, _ = built
    names = cs.names(k)
    with ThreadPoolExecutor(6) as ex:
        got = list(ex.map(lambda n: oracle.kosk_verify(k, b["cases"][n][1], b["cases"][n][0]), names))
    for name, (ok, why) in zip(names, got):
        assert not ok and reason_bit(why) == min(cs.CATALOGUE[name][0]), (k, name, why)


def test_the_hook_counts_every_check(oracle):
    """two plain tampers in different checks of one proof: both bits show, with their counts; the stopping verifier names the first"""
    k = 3
    pk, pi = cs.build(oracle, k)["honest"]
    t = cs.case(k, cs.case(k, pi, "ntt_s:i=0,j=0"), "sr_er:side=e,i=L,pos=1303")
    t = cs.case(k, t, "a_sr:i=L,j=149")
    ok, sites = oracle.kosk_verify_sites(k, t, pk)
    assert not ok and sites == [0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], sites
    ok, why = oracle.kosk_verify(k, t, pk)
    assert not ok and why == "e + r share error at %d." % (cs.opened_and_rest(k, pi)[1][1303] + 256), why
    # a byte of a hashed field: the relation checks hold, only I' == I fails -- at many positions of the list, each one counted
    h = bytearray(pi)
    h[oracle.params(k).off[23]] ^= 1
    ok, sites = oracle.kosk_verify_sites(k, bytes(h), pk)
    assert not ok and sites[:11] == [0] * 11 and sites[11] > 100, sites


def test_malformed_list_still_stops(oracle):
    k = 2
    pk, pi = cs.build(oracle, k)["honest"]
    o = oracle.params(k).off[cs.F_I]
    t = bytearray(cs.case(k, pi, "ntt_s:i=0,j=0"))
    t[o + 2:o + 4] = t[o:o + 2]  # I[1] = I[0]
    ok, sites = oracle.kosk_verify_sites(k, bytes(t), pk)
    assert not ok and sites == [1] + [0] * 11, sites
    assert oracle.kosk_verify(k, bytes(t), pk) == (False, "malformed opened-party list at 1")
