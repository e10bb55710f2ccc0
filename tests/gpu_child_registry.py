"""Child-process cases of tests/test_gpu_32_registry.py (the verified-key registry): what needs an environment
variable or a handle of another kind than the module's."""
import os

from tests import kem_fixture as kf
from tests import registry_cases as rc


def _refused(fn, text):
    from mpcith_kyber_kosk_amd import api
    try:
        fn()
    except api.KoskError as e:
        assert text in str(e), str(e)
        return str(e)
    raise AssertionError("not refused: " + text)


def per_lane_admission(k=3):
    """run with KOSK_DEBUG_KEM_WAVE_MAX=0: admissions of 3 and 65 keys on the per-lane layout of k_registry_admit (what more than
    KEM_WAVE_MAX keys use): read against hashlib, kosk_kem_enc_slots against the fixture"""
    assert os.environ.get("KOSK_DEBUG_KEM_WAVE_MAX") == "0"
    from mpcith_kyber_kosk_amd import api
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(rc.EDGE_CAPACITY)
    for n in (3, 65):
        idx = list(range(n))
        slots = [rc.edge_slot(b) for b in idx]
        ctx.registry_admit([rc.pks(k)[i] for i in idx], slots)
        assert ctx.registry_level() == (n, rc.EDGE_CAPACITY)
        rc.check_read(ctx, k, idx, slots)
        rc.check_enc(ctx, k, idx, slots)
        ctx.registry_evict(slots)
        assert ctx.registry_level() == (0, rc.EDGE_CAPACITY)
    assert ctx.path_count(api.Kosk.PATH_REGISTRY_ADMIT) == 2
    ctx.close()
    print("per_lane_admission ok %d" % k)


def cohort_member(k=2):
    """a cohort member admits explicitly and encapsulates by slot, unmerged; kosk_registry_admit_verified refuses there"""
    from mpcith_kyber_kosk_amd import api
    ctx = api.Kosk(kyber_k=k, max_batch=3, combine=2)
    idx = [5, 2, 97, 24, 0]
    slots = [rc.slot(i) for i in idx]
    ctx.registry_reserve(rc.CAPACITY)
    ctx.registry_admit([rc.pks(k)[i] for i in idx], slots)
    rc.check_read(ctx, k, idx, slots)
    cts, sss = rc.check_enc(ctx, k, idx, slots)
    assert (cts, sss) == ctx.kem_enc([rc.pks(k)[i] for i in idx], [rc.messages(k)[i] for i in idx])
    before = rc.counts(ctx, api)
    assert before[:2] == (1, 1) and before[5:] == (5, rc.CAPACITY)
    msg = _refused(lambda: ctx.registry_admit_verified([1, 2, 3]), "not available with call combining")
    assert "kosk_registry_admit_verified" in msg and rc.counts(ctx, api) == before
    ctx.close()
    print("cohort_member ok %d" % k)


def admit_verified_refused_with_two_streams(k=2):
    from mpcith_kyber_kosk_amd import api
    ctx = api.Kosk(kyber_k=k, max_batch=3, streams=2)
    ctx.registry_reserve(8)
    before = rc.counts(ctx, api)
    msg = _refused(lambda: ctx.registry_admit_verified([1, 2, 3]), "needs streams = 1")
    assert "kosk_registry_admit_verified" in msg and rc.counts(ctx, api) == before
    ctx.close()
    print("admit_verified_refused_with_two_streams ok %d" % k)


def block_limit_leaves_the_slots_empty(k=3):
    """run with KOSK_DEBUG_XOF_BLOCKS=1: gen_matrix reaches its block limit inside an admission -- -1 "block limit", the slots it named
    empty and zero, `used` unchanged, both layouts"""
    assert os.environ.get("KOSK_DEBUG_XOF_BLOCKS") == "1"
    from mpcith_kyber_kosk_amd import api
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.registry_reserve(rc.EDGE_CAPACITY)
    for n in (3, rc.WAVE_MAX + 1):
        idx = [b % kf.ITEMS for b in range(n)]
        slots = [rc.edge_slot(b) for b in range(n)]
        _refused(lambda: ctx.registry_admit([rc.pks(k)[i] for i in idx], slots), "block limit")
        assert ctx.registry_level() == (0, rc.EDGE_CAPACITY)
        probe = [slots[0], slots[-1]]
        assert ctx.registry_read(probe) == ([0, 0], [bytes(ctx.pk_bytes)] * 2, [bytes(32)] * 2)
        cts, sss, done = ctx.kem_enc_slots(probe, [rc.messages(k)[0]] * 2)
        assert done == [False, False] and cts == [bytes(kf.CT_BYTES[k])] * 2 and sss == [bytes(32)] * 2
        assert ctx.secret_scan(rc.pks(k)[0][:32]) == 0
    assert ctx.path_count(api.Kosk.PATH_REGISTRY_ADMIT) == 2
    ctx.close()
    print("block_limit_leaves_the_slots_empty ok %d" % k)
