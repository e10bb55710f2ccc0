"""Child-process cases of tests/test_gpu_39_relying.py (the relying party): handles of another kind than the module's."""
import hashlib

from tests import registry_cases as rc
from tests import registry_sorted_model as sm
from tests import relying_cases as cases


def cohort_member(k=2):
    """a cohort member without a registry checks the crafted tables and encapsulates to proven keys, unmerged; the verdicts are the host
    function's and the counters move as on a plain handle"""
    from mpcith_kyber_kosk_amd import api
    ctx = api.Kosk(kyber_k=k, max_batch=3, combine=2)
    d = cases.D
    t = cases.path_table(k)
    slots, hs, paths, states = cases.path_args(t)
    assert ctx.regtree_check_paths(d, slots, hs, paths, t["root"], states=states) == cases.host_paths(api, t)
    p = cases.proof_table(k)
    want = cases.host_proofs(api, p)
    assert ctx.regsort_check_proofs(d, [c[1] for c in p["cases"]], [c[2] for c in p["cases"]], p["root"]) == want and set(want) == {0, 1, 2}
    n = 12
    pks = list(rc.pks(k)[:n])
    coins = list(rc.messages(k)[:n])
    key_paths = [paths[slots.index(rc.slot(i))] for i in range(n)]
    key_paths[3] = cases.flip(key_paths[3], 1000)
    pks[7] = pks[8]
    cts, sss, done = ctx.kem_enc_proven(d, pks, [rc.slot(i) for i in range(n)], key_paths, t["root"], coins)
    assert done == [i not in (3, 7) for i in range(n)]
    plain = ctx.kem_enc(pks, coins)
    for i in range(n):
        if done[i]:
            assert (cts[i], sss[i]) == (plain[0][i], plain[1][i]) and sss[i].hex() == rc.items(k)[i]["ss"], i
        else:
            assert cts[i] == bytes(len(plain[0][i])) and sss[i] == bytes(32), i
    ids = (api.Kosk.PATH_REGTREE_CHECK, api.Kosk.PATH_REGSORT_CHECK, api.Kosk.PATH_KEM_ENC_PROVEN, 12, api.Kosk.PATH_REGISTRY_TREE, api.Kosk.PATH_REGSORT_TREE)
    assert tuple(ctx.path_count(i) for i in ids) == (2, 1, 1, 1, 0, 0)
    assert ctx.registry_level() == (0, 0) and hashlib.sha3_256(pks[0]).digest() == hs[slots.index(rc.slot(0))] and sm.PRESENT in want
    ctx.close()
    print("cohort_member ok %d" % k)
