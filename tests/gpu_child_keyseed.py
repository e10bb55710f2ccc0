"""Multi-handle cases of the derived proofs (format kosk-keyseed-v1; tests/test_gpu_22_keyseed.py runs each in a fresh child process)."""
from tests import keyproof_cases as kc
from tests import keyseed_model as km


def cohort_members_derive(k=2, per=2, rounds=2):
    """combine = 2: both members call prove_keys(derived) and the staged form concurrently, member 1 armed and salted.  Every proof is the
    seeded proof of the model's seed; no derived call went through the combiner's merged runs."""
    import threading
    from mpcith_kyber_kosk_amd import api
    sks = [[kc.honest(k, 2 * t + b)[1] for b in range(per)] for t in range(2)]
    ctxs = [bytes([0x40 + b]) * 32 for b in range(per)]
    salts = [bytes([0x80 + b]) * 32 for b in range(per)]
    seeds = [[km.seed(k, sks[0][b]) for b in range(per)], [km.seed(k, sks[1][b], ctxs[b], salts[b]) for b in range(per)]]
    opts = dict(combine=2, combine_wait_us=2000000, combine_idle_us=1000000)
    hs = [api.Kosk(kyber_k=k, max_batch=per, **opts) for _ in range(2)]
    hs[1].set_contexts(ctxs)
    want = [hs[t].prove_keys(sks[t], seeds=seeds[t])[0] for t in range(2)]
    errs = []
    barrier = threading.Barrier(2)

    def worker(t):
        try:
            h = hs[t]
            sal = salts if t == 1 else None
            for r in range(rounds):
                barrier.wait()
                got, ok = h.prove_keys(sks[t], derived=True, salts=sal)
                assert ok == [True] * per and got == want[t], ("host", t, r)
                assert h.stage_prover_keys(sks[t], derived=True, salts=sal) == [True] * per
                h.prove_resident(per)
                assert h.fetch_proofs(per) == want[t], ("resident", t, r)
                assert h.verify_resident_pk(per) == [True] * per, ("bits", t, r)
        except Exception as e:  # noqa: BLE001
            errs.append((t, repr(e)))
            try:
                barrier.abort()
            except Exception:
                pass
    th = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
    [x.start() for x in th]; [x.join() for x in th]
    assert not errs, errs
    for t in range(2):
        assert hs[t].path_count(api.Kosk.PATH_KEYSEED) == 2 * rounds, (t, hs[t].path_count(api.Kosk.PATH_KEYSEED))
    for h in hs:
        h.close()
    print("cohort_members_derive ok", k)
