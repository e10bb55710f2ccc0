"""Cases of the offline bank with more than one handle (tests/test_gpu_31_bank.py runs each in a fresh child process)."""
from tests import bank_cases as bc


def _api():
    from mpcith_kyber_kosk_amd import api
    return api


def _raises(api, call, text):
    try:
        call()
    except api.KoskError as e:
        assert text in str(e), (text, str(e))
        return
    raise AssertionError("not refused: " + text)


def erasure():
    """the needle is the first 32 bytes of f[0] of the entry's tape (kosk_prepare_randomness on a second handle).  KOSK_WIPE_CALL: found
    after the fill (in the bank), and after the banked call as often as the non-banked call on the same tape leaves it; mode off:
    kosk_wipe_secrets gives level 0 and no hit, the next banked call fails with "bank is empty", a fill makes it work again"""
    api = _api()
    for k in bc.KS:
        n = 2
        other = api.Kosk(kyber_k=k, max_batch=bc.MAX_BATCH)
        tapes, sks = [bc.tape(k, 20 + i) for i in range(n)], bc.sks(k, n)
        needles = [other.prepare_randomness([bc.offline_compact(k, t)])[0][:32] for t in tapes]
        other.wipe_secrets()
        want, _ = other.prove_keys(sks, tapes=tapes)
        other.set_wipe(api.WIPE_CALL)
        other.prove_keys(sks, tapes=tapes)
        left_by_the_plain_call = [other.secret_scan(nd) for nd in needles]
        other.close()
        h = api.Kosk(kyber_k=k, max_batch=bc.MAX_BATCH)
        h.bank_reserve(bc.CAPACITY)
        h.set_wipe(api.WIPE_CALL)
        h.bank_fill(tapes=tapes)
        assert h.bank_level() == (n, bc.CAPACITY)
        seen = [h.secret_scan(nd) for nd in needles]
        assert seen == [1] * n, ("after the fill the rows are in the bank and nowhere else", seen)
        got, ok = h.prove_keys_banked(sks, tapes=tapes)
        assert ok == [True] * n and got == want
        left = [h.secret_scan(nd) for nd in needles]
        print("hits after the banked call", left, "after the plain call", left_by_the_plain_call)
        assert left == left_by_the_plain_call == [0] * n, (left, left_by_the_plain_call)
        # a call in that mode that consumes some entries leaves the others alone
        h.bank_fill(tapes=tapes)
        h.prove_keys_banked(sks[:1], tapes=tapes[:1])
        assert [h.secret_scan(nd) for nd in needles] == [0, 1] and h.bank_level() == (1, bc.CAPACITY)
        h.set_wipe(api.WIPE_OFF)
        h.bank_fill(tapes=tapes[:1])
        assert h.secret_scan(needles[0]) >= 1
        h.wipe_secrets()
        assert h.bank_level() == (0, bc.CAPACITY)
        assert [h.secret_scan(nd) for nd in needles] == [0] * n
        _raises(api, lambda: h.prove_keys_banked(sks, tapes=tapes), "bank is empty")
        _raises(api, lambda: h.stage_prover_keys_banked(sks, tapes=tapes), "bank is empty")
        h.bank_fill(tapes=tapes)
        got, ok = h.prove_keys_banked(sks, tapes=tapes)
        assert ok == [True] * n and got == want
        h.close()
        print("erasure ok", k)


def reserve_rules():
    api = _api()
    for k in bc.KS:
        tapes, sks = [bc.tape(k, 30 + i) for i in range(2)], bc.sks(k, 2)
        h = api.Kosk(kyber_k=k, max_batch=bc.MAX_BATCH)
        assert h.bank_level() == (0, 0)
        _raises(api, lambda: h.bank_fill(tapes=tapes), "no room")
        _raises(api, lambda: h.prove_keys_banked(sks, tapes=tapes), "bank is empty")
        _raises(api, lambda: h.bank_reserve(-1), "negative")
        want, _ = h.prove_keys(sks, tapes=tapes)
        h.bank_reserve(2)
        h.bank_fill(tapes=tapes[:1])
        _raises(api, lambda: h.bank_reserve(4), "not empty")
        _raises(api, lambda: h.bank_reserve(0), "not empty")
        assert h.bank_level() == (1, 2)
        got, _ = h.prove_keys_banked(sks[:1], tapes=tapes[:1])
        assert got == want[:1]
        h.bank_reserve(0)
        assert h.bank_level() == (0, 0)
        _raises(api, lambda: h.bank_fill(tapes=tapes), "no room")
        h.bank_reserve(3)
        assert h.bank_level() == (0, 3)
        h.bank_fill(tapes=tapes)
        got, _ = h.prove_keys_banked(sks, tapes=tapes)
        assert got == want
        h.close()
        two = api.Kosk(kyber_k=k, max_batch=bc.MAX_BATCH, streams=2)
        assert two.streams == 2
        _raises(api, lambda: two.bank_reserve(2), "needs streams = 1")
        _raises(api, lambda: two.bank_fill(tapes=tapes), "needs streams = 1")
        assert two.prove_keys(sks, tapes=tapes)[0] == want
        two.close()
        print("reserve_rules ok", k)


def existing_calls_unaffected():
    """after banked work kosk_verifiable_keygen_batch (and the split call on host structs) return what a fresh handle returns"""
    api = _api()
    for k in bc.KS:
        n = 3
        tapes, sks = [bc.tape(k, 40 + i) for i in range(n)], bc.sks(k, n)
        fresh = api.Kosk(kyber_k=k, max_batch=bc.MAX_BATCH)
        want = fresh.verifiable_keygen(tapes)
        want_keys = fresh.prove_keys(sks, tapes=tapes)
        fresh.close()
        h = api.Kosk(kyber_k=k, max_batch=bc.MAX_BATCH)
        h.bank_reserve(bc.CAPACITY)
        h.bank_fill(tapes=[bc.tape(k, 50 + i) for i in range(4)])
        h.prove_keys_banked(sks, tapes=tapes)
        assert h.verifiable_keygen(tapes) == want
        assert h.stage_prover_keys_banked(sks[:1], tapes=tapes[:1]) == [True]
        assert h.prove_keys(sks, tapes=tapes) == want_keys
        assert h.verifiable_keygen(tapes) == want
        h.close()
        print("existing_calls_unaffected ok", k)


def cohort_member(k=3):
    """combine = 2: a member's banked calls run unmerged on its own block and return what a plain handle returns"""
    api = _api()
    n = 3
    off, on, sks = [bc.tape(k, 60 + i, "off") for i in range(n)], [bc.tape(k, 60 + i, "on") for i in range(n)], bc.sks(k, n)
    plain = api.Kosk(kyber_k=k, max_batch=2)
    want, _ = plain.prove_keys(sks, tapes=[bc.splice(k, a, b) for a, b in zip(off, on)])
    plain.close()
    hs = [api.Kosk(kyber_k=k, max_batch=2, combine=2) for _ in range(2)]
    m = hs[1]
    m.bank_reserve(4)
    m.bank_fill(tapes=off)          # chunks of 2 + 1 on the member's block
    got, ok = m.prove_keys_banked(sks, tapes=on)
    assert ok == [True] * n and got == want
    assert m.combine_stats() == (0, 0)
    for h in hs:
        h.close()
    print("cohort_member ok", k)
