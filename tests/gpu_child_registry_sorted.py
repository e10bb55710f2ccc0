"""Child-process cases of tests/test_gpu_36_registry_sorted.py (the sorted tree): handles of another kind than the
module's."""
import hashlib

from tests import registry_cases as rc
from tests import registry_sorted_model as sm
from tests import registry_tree_model as tm


def cohort_member(k=2):
    """a cohort member takes the sorted root and proves absence and presence, unmerged; the counters move as on a plain handle"""
    from mpcith_kyber_kosk_amd import api
    ctx = api.Kosk(kyber_k=k, max_batch=3, combine=2)
    idx = [5, 2, 97, 24, 0]
    pks = [rc.pks(k)[i] for i in idx]
    hs = [hashlib.sha3_256(p).digest() for p in pks]
    slots = [6, 0, 3, 4, 1]
    ctx.registry_reserve(7)
    ctx.registry_admit(pks, slots)
    content = dict(zip(slots, hs))
    lv = sm.levels(k, 7, content)
    d = tm.depth(7)
    assert ctx.registry_sorted_root() == (sm.root(lv), 5, 7)
    queries = [bytes(32), b"\xff" * 32, hashlib.sha3_256(b"nobody").digest()]
    for h in hs:
        queries += [h] + sm.neighbours(h)
    kinds, records, root = ctx.registry_prove_absent(queries)
    assert root == sm.root(lv)
    for b, x in enumerate(queries):
        assert (kinds[b], records[b]) == sm.prove(k, 7, content, x, lv), b
        assert api.regsort_check_proof(k, d, x, records[b], root) == kinds[b] == (sm.PRESENT if x in hs else sm.ABSENT), b
    ids = (api.Kosk.PATH_REGSORT_SORT, api.Kosk.PATH_REGSORT_TREE, api.Kosk.PATH_REGSORT_PROVE, api.Kosk.PATH_REGISTRY_TREE,
           api.Kosk.PATH_REGISTRY_INDEX, api.Kosk.PATH_REGISTRY_FIND)
    assert tuple(ctx.path_count(i) for i in ids) == (2, 1, 1, 0, 0, 0)
    ctx.registry_evict([3])
    del content[3]
    kinds, records, root = ctx.registry_prove_absent([hs[2]])
    assert root == sm.root(sm.levels(k, 7, content)) and kinds == [sm.ABSENT]
    assert api.regsort_check_proof(k, d, hs[2], records[0], root) == sm.ABSENT
    ctx.close()
    print("cohort_member ok %d" % k)
