"""Multi-handle / multi-thread / environment cases of the erasure calls (tests/test_gpu_24_wipe.py runs each in a fresh child process)."""
import os

from tests import wipe_cases as wc


def _gone(h, needles, what):
    left = {n.name: h.secret_scan(n.data) for n in needles}
    assert not any(left.values()), (what, left)


def _there(h, needles, what):
    seen = {n.name: h.secret_scan(n.data) for n in needles}
    assert all(v >= 1 for v in seen.values()), (what, seen)


def cohort_member_wipes_its_own_block(k=3, per=2, rounds=3):
    """combine = 3: members 0 and 1 plain, member 2 in KOSK_WIPE_CALL, all calling concurrently.  Every caller gets the bytes of an
    uncombined handle; member 2's calls never count as served by the combiner, members 0 and 1 still merge with each other; after its
    call member 2's needles are gone through its own handle while a neighbour's are still found through the neighbour's: a view wipes
    its own block of the shared workspace and nothing else.  Destroying the three members completes."""
    import threading
    from mpcith_kyber_kosk_amd import api
    tapes = [[wc.tape(k, 200 + t * per + b) for b in range(per)] for t in range(3)]
    plain = api.Kosk(kyber_k=k, max_batch=per)
    want = []
    for t in range(3):
        plain.verifiable_keygen_resident(tapes[t])
        want.append((plain.keys(per), plain.fetch_proofs(per)))
    opts = dict(combine=3, combine_wait_us=300000, combine_idle_us=150000)
    hs = [api.Kosk(kyber_k=k, max_batch=per, **opts) for _ in range(3)]
    hs[2].set_wipe(api.WIPE_CALL)
    errs = []
    barrier = threading.Barrier(3)

    def worker(t):
        try:
            h = hs[t]
            for r in range(rounds):
                barrier.wait()
                h.verifiable_keygen_resident(tapes[t])
                assert h.keys(per) == want[t][0], ("keys", t, r)
                assert h.verify_resident_pk(per) == [True] * per, ("bits", t, r)
                assert h.fetch_proofs(per) == want[t][1], ("proofs", t, r)
        except Exception as e:  # noqa: BLE001
            errs.append((t, repr(e)))
            try:
                barrier.abort()
            except Exception:
                pass
    th = [threading.Thread(target=worker, args=(t,)) for t in range(3)]
    [x.start() for x in th]; [x.join() for x in th]
    assert not errs, errs
    assert hs[2].combine_stats() == (0, 0), hs[2].combine_stats()   # never served by a merged run
    for t in (0, 1):
        c, m = hs[t].combine_stats()
        assert m > c, (t, c, m)                                        # the other two did merge (with each other)
    needles = [wc.tape_needles(tapes[t][-1]) + wc.sk_needles(want[t][0][1][-1]) for t in range(3)]
    _gone(hs[2], needles[2], "the wiping member, through its own handle")
    for t in (0, 1):
        _there(hs[t], needles[t], "neighbour %d, through its own handle" % t)
        _gone(hs[t], needles[1 - t], "a handle sees its own block only")
    assert hs[2].path_count(api.Kosk.PATH_WIPE) == rounds
    # once more, alone: the neighbours' blocks are as they were
    hs[2].verifiable_keygen_resident(tapes[2])
    _gone(hs[2], needles[2], "the wiping member, second time")
    for t in (0, 1):
        _there(hs[t], needles[t], "neighbour %d after the wiping member's call" % t)
        assert hs[t].fetch_proofs(per) == want[t][1]
    # an explicit wipe of member 0 leaves member 1's block alone
    hs[0].wipe_secrets()
    _gone(hs[0], needles[0], "member 0 after kosk_wipe_secrets")
    _there(hs[1], needles[1], "member 1 after member 0's wipe")
    assert hs[0].fetch_proofs(per) == want[0][1] and hs[0].verify_resident_pk(per) == [True] * per
    for h in hs:
        h.close()
    plain.verifiable_keygen_resident(tapes[0])
    assert plain.fetch_proofs(per) == want[0][1]
    plain.close()
    print("cohort_member_wipes_its_own_block ok", k)


def two_streams(k=3):
    """streams = 2: every sub-context is wiped, by kosk_wipe_secrets and at the end of a call under KOSK_WIPE_CALL, chunked or not"""
    from mpcith_kyber_kosk_amd import api
    plain = api.Kosk(kyber_k=k, max_batch=4)
    h = api.Kosk(kyber_k=k, max_batch=4, streams=2)
    assert h.streams == 2
    needles, res = wc.plant_keygen_tapes(h, n=4, first=300)
    first = wc.tape_needles(wc.tape(k, 300)) + wc.sk_needles(res[1][0])  # sub-context 0 served proofs 0 and 1, sub-context 1 the others
    _there(h, needles + first, "mode off")
    assert res == wc.plant_keygen_tapes(plain, n=4, first=300)[1]
    h.wipe_secrets()
    _gone(h, needles + first, "kosk_wipe_secrets on two sub-contexts")
    assert h.path_count(api.Kosk.PATH_WIPE) == 2
    h.set_wipe(api.WIPE_CALL)
    needles, res = wc.plant_keygen_tapes(h, n=4, first=310)
    _gone(h, needles + wc.tape_needles(wc.tape(k, 310)) + wc.sk_needles(res[1][0]), "WIPE_CALL on two sub-contexts")
    assert res == wc.plant_keygen_tapes(plain, n=4, first=310)[1]
    needles, res = wc.plant_prove_keys_seeded(h, n=5)  # chunks of 2, 2 and 1 dealt to the two lanes
    _gone(h, needles + wc.sk_needles(wc.honest_keys(k, 5)[1][0]) + [wc.Needle("seed", wc.seed(40))], "chunked call on two sub-contexts")
    assert res == wc.plant_prove_keys_seeded(plain, n=5)[1]
    needles, res = wc.plant_kem_dec(h)
    _gone(h, needles, "KEM call on sub-context 0")
    h.close(); plain.close()
    print("two_streams ok", k)


def error_path(k=3):
    """KOSK_DEBUG_XOF_BLOCKS=1 forces gen_matrix's block limit: the calls return -1 after their inputs were uploaded.  Under
    KOSK_WIPE_CALL the needles are gone after that return; with the mode off they are still there (so the check means something)"""
    from mpcith_kyber_kosk_amd import api
    os.environ["KOSK_DEBUG_XOF_BLOCKS"] = "1"
    try:
        w, off = api.Kosk(kyber_k=k, max_batch=2), api.Kosk(kyber_k=k, max_batch=2)
    finally:
        del os.environ["KOSK_DEBUG_XOF_BLOCKS"]
    w.set_wipe(api.WIPE_CALL)
    tapes = [wc.tape(k, 400 + b) for b in range(2)]
    coins = [wc.coins64(50 + b) for b in range(3)]
    _pks, sks = wc.honest_keys(k, 2)
    for h in (w, off):
        check = _gone if h is w else _there
        for call in (lambda: h.verifiable_keygen(tapes), lambda: h.verifiable_keygen_resident(tapes)):
            try:
                call()
                raise AssertionError("the forced block limit did not fail the call")
            except api.KoskError as e:
                assert "block limit" in str(e), str(e)
            check(h, wc.tape_needles(tapes[-1]), "key generation that failed")
        try:
            h.kem_keypair(coins=coins)
            raise AssertionError("the forced block limit did not fail the call")
        except api.KoskError as e:
            assert "block limit" in str(e), str(e)
        check(h, [wc.Needle("keypair: d", coins[-1][:32]), wc.Needle("keypair: z", coins[-1][32:])], "kem_keypair that failed")
        try:
            h.prove_keys(sks, tapes=tapes)
            raise AssertionError("the forced block limit did not fail the call")
        except api.KoskError as e:
            assert "block limit" in str(e), str(e)
        check(h, wc.sk_needles(sks[-1]) + wc.tape_needles(tapes[-1], key_seed=False), "prove_keys that failed")
    w.close(); off.close()
    print("error_path ok", k)
