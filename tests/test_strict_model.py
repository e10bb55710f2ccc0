"""tests/strict_model.py pinned to the oracle on the CPU: which u16 records of a proof image the reference's verifier reads.

The strict default of the GPU verifier rejects a u16 >= q exactly in those records, and the oracle -- the reference's arithmetic --
cannot decide strict cases; what it can decide is whether a record is READ: another canonical residue in a read record breaks a
check, in an unread one nothing looks.  tests/test_gpu_15_strict_encoding.py takes its expectations from the model pinned here."""
import pytest

from tests import strict_model as sm


def test_widths_and_limits_of_the_model(oracle):
    p = oracle.params(2)
    _, _, pi, _, _ = oracle.verifiable_keygen(2, oracle.tape_bytes_for(2, sm.TAPE))
    m = sm.ReadSet(p, *sm.opened_list(p, pi))
    assert len(sm.U16_FIELDS) == 21 and len(sm.LIMITED_FIELDS) == 7
    # M, M, NCHK, NCHK, nine fields of K, four of K E, four of K Z
    assert [m.width[f] for f in sm.U16_FIELDS] == [75, 75, 70, 70] + [2] * 9 + [14] * 4 + [12] * 4
    assert m.limit_records(8) == (406, 407) and m.limit_records(21) == (812, 813)
    lo, hi = m.limit_records(2)
    assert hi == lo + 1 and m.rest[lo] < 407 <= m.rest[hi]
    assert m.strict_expectation(pi) == {}
    # one element >= q in a read record is counted under its field, one in an unread record is not
    assert m.strict_expectation(m.put(pi, 8, m.index(8, 406, -1), sm.Q)) == {8: 1}
    assert m.strict_expectation(m.put(pi, 8, m.index(8, 407, 0), 0xFFFF)) == {}
    assert m.strict_expectation(m.put(pi, 2, m.index(2, hi, 0), sm.Q)) == {}
    assert m.strict_expectation(m.put(pi, 2, m.index(2, lo, 0), sm.Q)) == {2: 1}


@pytest.mark.parametrize("k", [2, 3, 4])
def test_oracle_rejects_exactly_the_records_the_model_calls_read(k, oracle):
    """Honest oracle proof of tape 133; at the first and last record of every u16 field and on both sides of every limit (the largest
    i with rest[i] < 407 and the next; records 406 / 407; 812 / 813), first and last element: (v + 1) % q, another canonical residue.
    The oracle rejects exactly where read() is true."""
    pk, pi, m, cases, bits = sm.boundary_set(oracle, k)
    assert oracle.kosk_verify(k, pi, pk)[0]
    assert len(cases) == 2 * (2 * 21 + 2 * 7) == len(set(cases))
    for f in sm.LIMITED_FIELDS:
        lo, hi = m.limit_records(f)
        assert m.read(f, lo) and not m.read(f, hi) and not m.read(f, sm.NREST - 1)
    assert m.limit_records(8) == m.limit_records(15) == m.limit_records(16) == (406, 407)
    assert m.limit_records(21) == m.limit_records(22) == (812, 813)
    wrong = [(f, rec, elem, m.read(f, rec), ok) for (f, rec, elem), ok in zip(cases, bits) if ok == m.read(f, rec)]
    assert not wrong, "K=%d (field, record, element, model says read, oracle accepts): %s" % (k, wrong)
    assert sum(bits) == 2 * (7 + 7)  # last record and first unread record of the seven limited fields, two elements each
