"""Child-process case of tests/test_gpu_15_strict_encoding.py (cohort handles live in a fresh process, like every multi-handle case)."""


def merged_runs_keep_their_mode(rounds=4):
    """Two default handles with combine=2 form a cohort; a strict_encoding=0 handle with the same combine, created BETWEEN them, must land
    in another one (kosk_mi355x.h: a cohort is formed by handles whose options agree).  Three caller threads each stage the same three
    K = 3 proofs -- + q in a read record, + q in an unread record, honest -- and verify them with merged calls: both default callers
    get [False, True, True] with fail bit 0 on the first from runs that served the two of them, the reference-following caller
    gets the reference's answer from runs that served nobody else."""
    import threading
    from mpcith_kyber_kosk_amd import api
    from tests import oracle_lib as oracle
    from tests.test_gpu_15_strict_encoding import WAYS_K as k, WAYS_TAPE, ways_in_cases
    # a member counts as expected for 2 s after its last call: the barrier below brings the callers back well within that, so from
    # the second round on whoever posts first waits for its neighbour
    opts = dict(combine=2, combine_wait_us=500000, combine_idle_us=2000000)
    a = api.Kosk(kyber_k=k, max_batch=3, **opts)
    lax = api.Kosk(kyber_k=k, max_batch=3, strict_encoding=0, **opts)
    b = api.Kosk(kyber_k=k, max_batch=3, **opts)
    hs = [a, b, lax]
    pks, _, pis = a.verifiable_keygen([oracle.tape_bytes_for(k, WAYS_TAPE)])
    pks = pks * 3
    cases, _ = ways_in_cases(oracle, pks[0], pis[0])
    want = [False, True, True]
    assert [oracle.kosk_verify(k, t, pks[0])[0] for t in cases] == want  # the read record is an s + r share: compared raw
    errs = []
    barrier = threading.Barrier(len(hs))

    def worker(t):
        try:
            h = hs[t]
            h.stage_verifier_inputs(cases, pks)
            for r in range(rounds):
                barrier.wait()
                bits = h.verify_resident_pk(3, pks=pks)
                masks = h.fail_masks(3)
                assert bits == want and masks[0] != 0 and masks[1:] == [0, 0], (t, r, bits, masks)
                assert (masks[0] & 1) == (h is not lax), (t, r, hex(masks[0]))  # malformed by default; the reference's own check otherwise
        except Exception as e:  # noqa: BLE001
            errs.append((t, repr(e)))
            try:
                barrier.abort()
            except Exception:
                pass
    ths = [threading.Thread(target=worker, args=(t,)) for t in range(len(hs))]
    for x in ths:
        x.start()
    for x in ths:
        x.join()
    assert not errs, errs
    (ca, ma), (cb, mb), (cl, ml) = (h.combine_stats() for h in hs)
    assert ca == cb == cl == rounds, (ca, cb, cl)
    assert ml == cl, "the strict_encoding=0 handle was served by a run with other members: %d calls, %d members" % (cl, ml)
    assert ma <= 2 * ca and mb <= 2 * cb and ma + mb > ca + cb, "the two default handles never merged: %s" % ((ca, ma, cb, mb),)
    for h in hs:
        h.close()
    print("merged_runs_keep_their_mode ok")
