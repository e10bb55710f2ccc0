"""Cases of buffer ownership that need several handles or a cohort (tests/test_gpu_34_ownership.py runs each in a fresh child
process).  K = 2 and max_batch = 2 throughout, except the inventory numbers, which are taken at K = 2, 3, 4."""
import json

from tests import bank_cases as bc
from tests import kem_fixture as kf

K, MAX_BATCH = 2, 2


def _api():
    from mpcith_kyber_kosk_amd import api
    return api


def _member(api, k=K):
    return api.Kosk(kyber_k=k, max_batch=MAX_BATCH, combine=3, combine_wait_us=2000, combine_idle_us=500)


def _try(api, call):
    """'ok', or the refusal's text"""
    try:
        call()
        return "ok"
    except api.KoskError as e:
        return str(e)


def _tapes(k, first, n=2):
    return [bc.tape(k, first + i, "own") for i in range(n)]


def _prove_and_verify(h, tapes):
    pks, sks, pis = h.verifiable_keygen(tapes)
    assert h.verify(pis, pks) == [True] * len(tapes)
    return pks, sks, pis


def cohort_isolation():
    """Every per-handle feature on member 1 of three; members 0 and 2 see none of it.  Prints what member 1's calls returned (the test
    holds the parent commit's answers), then all three members prove and verify what an uncombined handle does on the same tapes."""
    api = _api()
    plain = api.Kosk(kyber_k=K, max_batch=MAX_BATCH)
    want = [_prove_and_verify(plain, _tapes(K, 10 * m)) for m in range(3)]
    plain.close()
    hs = [_member(api) for _ in range(3)]
    m1 = hs[1]
    pk0, sk0 = bc.pks(K, 1)[0], bc.sks(K, 1)[0]
    out = {}
    out["kem_key_set"] = _try(api, lambda: m1.kem_key_set(pk=pk0))
    out["registry_reserve"] = _try(api, lambda: m1.registry_reserve(4))
    out["bank_reserve"] = _try(api, lambda: m1.bank_reserve(2))
    out["set_contexts"] = _try(api, lambda: m1.set_contexts([bytes([7]) * 32, bytes([9]) * 32]))
    out["compact_fetch"] = _try(api, lambda: (m1.verifiable_keygen_resident(_tapes(K, 40)), m1.fetch_proofs_compact(2)))
    out["transcode"] = _try(api, lambda: m1.transcode([want[1][2][0]], api.FMT_IMAGE, api.FMT_COMPACT))
    out["witness_from_sk"] = _try(api, lambda: m1.witness_from_sk([sk0]))
    print("outcomes " + json.dumps(out, sort_keys=True))
    state = {"kem_key_state": m1.kem_key_state(), "registry": m1.registry_level()[1], "bank": m1.bank_level()[1]}
    print("member1 " + json.dumps(state, sort_keys=True))
    for i in (0, 2):
        h = hs[i]
        assert h.kem_key_state() == api.KEM_KEY_NONE, i
        assert h.registry_level() == (0, 0) and h.bank_level() == (0, 0), i
        assert not any(h.path_counts().values()), (i, h.path_counts())
    if out["set_contexts"] == "ok":
        m1.clear_contexts()  # the comparison below is with unbound proofs
    for m, h in enumerate(hs):
        assert _prove_and_verify(h, _tapes(K, 10 * m)) == want[m], m
    for h in hs:
        h.close()
    print("cohort_isolation ok")


def teardown_orders():
    """members destroyed in the order 1, 0, 2 (the last one frees the arena), the cohort created again: the same bytes; a handle of two
    sub-contexts created, used and destroyed twice"""
    api = _api()
    plain = api.Kosk(kyber_k=K, max_batch=MAX_BATCH)
    want = [_prove_and_verify(plain, _tapes(K, 10 * m)) for m in range(3)]
    plain.close()
    for rnd in range(2):
        hs = [_member(api) for _ in range(3)]
        for m, h in enumerate(hs):
            assert _prove_and_verify(h, _tapes(K, 10 * m)) == want[m], (rnd, m)
        hs[1].witness_from_sk(bc.sks(K, 1))  # a private buffer of a member goes with the member
        for i in (1, 0, 2):
            hs[i].close()
    for rnd in range(2):
        two = api.Kosk(kyber_k=K, max_batch=MAX_BATCH, streams=2)
        assert two.streams == 2
        assert _prove_and_verify(two, _tapes(K, 0)) == want[0], rnd
        two.close()
    print("teardown_orders ok")


def inventory_numbers():
    """(bytes, regions) of the secret HBM regions (kosk_wipe_timing) at K = 2, 3, 4 in three states of a plain handle and of member 1 of a
    cohort of three: fresh; after one keygen + verify; after additionally a KEM call of n = 1, witness_from_sk of n = 1 and bank_reserve(2).
    A call the library refuses is recorded by its text"""
    api = _api()
    out = {}
    for k in bc.KS:
        rec = {}
        for who in ("plain", "member"):
            hs = [api.Kosk(kyber_k=k, max_batch=MAX_BATCH)] if who == "plain" else [_member(api, k) for _ in range(3)]
            h = hs[-1] if who == "plain" else hs[1]
            states = []

            def measure():
                got = []
                why = _try(api, lambda: got.append(h.wipe_timing(reps=1)[2:]))
                states.append(list(got[0]) if why == "ok" else why)
            measure()
            _prove_and_verify(h, _tapes(k, 0))
            measure()
            pk, sk = kf.keypair(k, 0)
            extra = [_try(api, lambda: h.kem_enc([pk], [kf.message(k, 0)])), _try(api, lambda: h.witness_from_sk(bc.sks(k, 1))),
                     _try(api, lambda: h.bank_reserve(2))]
            measure()
            rec[who] = {"states": states, "extra_calls": extra}
            for x in hs:
                x.close()
        out["k%d" % k] = rec
    print("inventory " + json.dumps(out, sort_keys=True))
