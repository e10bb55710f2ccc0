"""Child-process case of tests/test_gpu_38_registry_monitor.py (the registry monitor): a handle of another kind than
the module's."""
from tests import registry_history_model as hm
from tests import registry_monitor_cases as mc
from tests import registry_monitor_model as mm


def cohort_member(k=2):
    """a cohort member replays a log, unmerged: verdict, head, roots, table and level against the model; then a rejected log and a new
    reserve; the counters move as on a plain handle"""
    from mpcith_kyber_kosk_amd import api
    ctx = api.Kosk(kyber_k=k, max_batch=3, combine=2)
    events = mc.scripted(k)
    n = len(events)
    cut = 9
    ctx.monitor_reserve(8, n)
    assert ctx.monitor_feed(events[:cut]) == (True, -1, api.MONITOR_OK)
    assert ctx.monitor_feed(b"".join(events[cut:])) == (True, -1, api.MONITOR_OK)
    table = mm.replay(k, 8, events)[3]
    assert ctx.monitor_level() == (n, n, len(table), 8, False)
    assert ctx.monitor_head() == (hm.mth(k, [hm.leaf(k, e) for e in events]), n)
    assert ctx.monitor_roots() == mm.roots(k, 8, table)
    assert ctx.monitor_read(list(range(8))) == ([int(s in table) for s in range(8)], [table.get(s, bytes(32)) for s in range(8)])
    ops = [e[0] for e in events[:cut]], [e[0] for e in events[cut:]]
    segments = sum(sum(1 for i, op in enumerate(part) if op != 3 and (i == 0 or part[i - 1] == 3)) for part in ops)
    assert tuple(ctx.path_count(i) for i in (42, 43, 44, 45)) == (segments, 2 * segments, segments + 4, 4)
    name, bad, why = mc.checkpoint_defects(events, n - 1)[6]
    ctx.monitor_reserve(8, n)
    assert ctx.monitor_feed(bad) == (False, n - 1, why) == (False, n - 1, api.MONITOR_CP_SORTED_ROOT), name
    size, _, used, _, failed = ctx.monitor_level()
    assert failed and size <= n - 1 and used == len(mm.replay(k, 8, events[:size])[3])
    try:
        ctx.monitor_feed(events[:1])
    except api.KoskError as e:
        assert str(e).startswith("monitor_feed: kosk_monitor_feed: ") and "failed" in str(e), str(e)
    else:
        raise AssertionError("a failed monitor took a feed")
    ctx.close()
    print("cohort_member ok %d" % k)
