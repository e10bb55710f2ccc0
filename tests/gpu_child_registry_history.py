"""Child-process cases of tests/test_gpu_37_registry_history.py (the registry history): what needs an environment
variable or a handle of another kind than the module's."""
import hashlib
import os

from tests import registry_cases as rc
from tests import registry_history_model as hm
from tests import registry_sorted_model as sm
from tests import registry_tree_model as tm


def cohort_member(k=2):
    """a cohort member keeps a history, takes heads and proves events and consistency, unmerged; the counters move as on a plain handle"""
    from mpcith_kyber_kosk_amd import api
    ctx = api.Kosk(kyber_k=k, max_batch=3, combine=2)
    idx = [5, 2, 97, 24, 0]
    pks = [rc.pks(k)[i] for i in idx]
    hs = [hashlib.sha3_256(p).digest() for p in pks]
    slots = [6, 0, 3, 4, 1]
    ctx.registry_reserve(7)
    ctx.registry_history_reserve(20)
    log = hm.Log(k, 7)
    ctx.registry_admit(pks, slots)
    log.admit(list(zip(slots, hs)))
    ctx.registry_evict([3, 5])
    log.evict([3, 5])
    content = dict(log.table)
    assert ctx.registry_history_checkpoint() == log.checkpoint(tm.root(tm.levels(k, 7, content)), sm.root(sm.levels(k, 7, content))) == 6
    assert ctx.registry_history_read() == log.events and hm.replay(log.events) == content
    n = len(log.events)
    leaves = log.leaves()
    head = hm.mth(k, leaves)
    assert ctx.registry_history_head() == (head, n)
    got, records, root = ctx.registry_history_prove_events(list(range(n)))
    assert got == leaves and root == head
    for i, rec in enumerate(records):
        assert rec == hm.inclusion_record(k, i, leaves) and api.reghist_root_from_path(i, n, leaves[i], rec) == head, i
    records, root = ctx.registry_history_prove_consistency(list(range(n + 1)))
    for m, rec in enumerate(records):
        assert rec == hm.consistency_record(k, m, leaves) and api.reghist_check_consistency(m, n, hm.mth(k, leaves[:m]), head, rec), m
    # three appends of one group each, one frontier, two proving launches; the checkpoint built both state trees once
    ids = (38, 39, 40, 41, api.Kosk.PATH_REGISTRY_TREE, api.Kosk.PATH_REGSORT_TREE, api.Kosk.PATH_REGSORT_PROVE, api.Kosk.PATH_REGISTRY_PATH)
    assert tuple(ctx.path_count(i) for i in ids) == (3, 3, 1, 2, 1, 1, 0, 0)
    ctx.close()
    print("cohort_member ok %d" % k)


def block_limit_appends_nothing(k=3):
    """run with KOSK_DEBUG_XOF_BLOCKS=1: an admission into empty slots that fails with "block limit" leaves the history as it was"""
    assert os.environ.get("KOSK_DEBUG_XOF_BLOCKS") == "1"
    from mpcith_kyber_kosk_amd import api
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(8)
    ctx.registry_history_reserve(16)
    try:
        ctx.registry_admit([rc.pks(k)[i] for i in range(3)], [1, 4, 6])
    except api.KoskError as e:
        assert "block limit" in str(e), str(e)
    else:
        raise AssertionError("the forced block limit did not fail the call")
    assert ctx.registry_level() == (0, 8) and ctx.registry_history_level() == (0, 16)
    assert ctx.registry_history_head() == (hm.empty(k), 0) and ctx.path_count(38) == 0
    assert ctx.registry_history_checkpoint() == 0
    content = {}
    assert ctx.registry_history_read() == [hm.record(3, 0, 8, tm.root(tm.levels(k, 8, content)), sm.root(sm.levels(k, 8, content)))]
    ctx.close()
    print("block_limit_appends_nothing ok %d" % k)
