"""Child-process cases of tests/test_gpu_35_registry_tree.py (the registry tree): handles of another kind than the
module's."""
import hashlib

from tests import registry_cases as rc
from tests import registry_tree_model as tm


def cohort_member(k=2):
    """a cohort member takes the root and proves by slot and by fingerprint, unmerged; the counters move as on a plain handle"""
    from mpcith_kyber_kosk_amd import api
    ctx = api.Kosk(kyber_k=k, max_batch=3, combine=2)
    idx = [5, 2, 97, 24, 0]
    pks = [rc.pks(k)[i] for i in idx]
    hs = [hashlib.sha3_256(p).digest() for p in pks]
    slots = [6, 0, 3, 4, 1]
    ctx.registry_reserve(7)
    ctx.registry_admit(pks, slots)
    lv = tm.levels(k, 7, dict(zip(slots, hs)))
    d = tm.depth(7)
    assert ctx.registry_root() == (tm.root(lv), 5, 7)
    states, got_h, paths, root = ctx.registry_prove_slots(list(range(7)))
    assert root == tm.root(lv) and states == [1, 1, 0, 1, 1, 0, 1]
    for s in range(7):
        h = dict(zip(slots, hs)).get(s)
        assert got_h[s] == (h or bytes(32)) and paths[s] == tm.path(lv, s), s
        assert api.regtree_root_from_path(k, d, s, h, paths[s]) == root
    absent = hashlib.sha3_256(b"nobody").digest()
    found, paths, done, root = ctx.registry_prove_peers(hs + [absent])
    assert found == slots + [-1] and done == [True] * 5 + [False] and root == tm.root(lv)
    assert paths == [tm.path(lv, s) for s in slots] + [bytes(32 * d)]
    ids = (api.Kosk.PATH_REGISTRY_TREE, api.Kosk.PATH_REGISTRY_SUBTREES, api.Kosk.PATH_REGISTRY_PATH, api.Kosk.PATH_REGISTRY_INDEX,
           api.Kosk.PATH_REGISTRY_FIND)
    assert tuple(ctx.path_count(i) for i in ids) == (1, 1, 2, 1, 1)
    ctx.registry_evict([3])
    assert ctx.registry_root()[0] == tm.root(tm.levels(k, 7, {s: h for s, h in zip(slots, hs) if s != 3}))
    ctx.close()
    print("cohort_member ok %d" % k)
