"""Multi-handle / multi-thread cases of the context-bound proofs (tests/test_gpu_18_bound.py runs each in a fresh child process)."""
from tests import bound_oracle as bo
from tests import oracle_lib as oracle


def cohort_armed_member(k=2, per=2, rounds=3):
    """combine = 3: members 0 and 1 unarmed, member 2 armed, all calling concurrently.  Every proof equals its model (the plain oracle for
    the unarmed members, the derived model for the armed one), the armed member's calls all ran alone, the unarmed members still merged."""
    import threading
    from mpcith_kyber_kosk_amd import api
    tapes = [[oracle.tape_bytes_for(k, t * per + b) for b in range(per)] for t in range(3)]
    ctxs = [bo.context_of(100 + b) for b in range(per)]
    want = []
    for t in range(3):  # the models first, on this thread: the derived model's binding value is a global
        if t < 2:
            rows = [oracle.verifiable_keygen(k, tp)[:3] for tp in tapes[t]]
        else:
            rows = [bo.case(k, t * per + b, ctxs[b]) for b in range(per)]
        want.append(([r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]))
    opts = dict(combine=3, combine_wait_us=2000000, combine_idle_us=1000000)
    hs = [api.Kosk(kyber_k=k, max_batch=per, **opts) for _ in range(3)]
    hs[2].set_contexts(ctxs)
    errs = []
    barrier = threading.Barrier(3)

    def worker(t):
        try:
            h = hs[t]
            for r in range(rounds):
                barrier.wait()
                h.verifiable_keygen_resident(tapes[t])
                assert h.keys(per) == (want[t][0], want[t][1]), ("keys", t, r)
                assert h.verify_resident_pk(per) == [True] * per, ("bits", t, r)
                assert h.fetch_proofs(per) == want[t][2], ("proofs", t, r)
        except Exception as e:  # noqa: BLE001
            errs.append((t, repr(e)))
            try:
                barrier.abort()
            except Exception:
                pass
    th = [threading.Thread(target=worker, args=(t,)) for t in range(3)]
    [x.start() for x in th]; [x.join() for x in th]
    assert not errs, errs
    c2, m2 = hs[2].combine_stats()
    assert c2 == 2 * rounds and m2 == c2, (c2, m2)          # every call of the armed member ran alone
    for t in (0, 1):
        c, m = hs[t].combine_stats()
        assert m > c, (t, c, m)                             # the unarmed members did merge (with each other)
    # disarmed, member 2 is a member like the others again: the plain oracle's bytes
    hs[2].clear_contexts()
    hs[2].verifiable_keygen_resident(tapes[2])
    assert hs[2].fetch_proofs(per) == [oracle.verifiable_keygen(k, tp)[2] for tp in tapes[2]]
    for h in hs:
        h.close()
    print("cohort_armed_member ok", k)
