"""Child-process cases of tests/test_gpu_33_registry_index.py (the registry by fingerprint): handles of another kind
than the module's."""
import hashlib

from tests import kem_fixture as kf
from tests import registry_cases as rc
from tests import registry_index_model as rm


def _refused(fn, text):
    from mpcith_kyber_kosk_amd import api
    try:
        fn()
    except api.KoskError as e:
        assert text in str(e), str(e)
        return str(e)
    raise AssertionError("not refused: " + text)


def cohort_member(k=2):
    """a cohort member enrols explicitly, finds and encapsulates to peers, unmerged; kosk_registry_enrol_verified refuses there, and on a
    handle with two streams"""
    from mpcith_kyber_kosk_amd import api
    ctx = api.Kosk(kyber_k=k, max_batch=3, combine=2)
    idx = [5, 2, 97, 24, 0]
    pks = [rc.pks(k)[i] for i in idx]
    hs = [hashlib.sha3_256(p).digest() for p in pks]
    ctx.registry_reserve(8)
    assert ctx.registry_enrol(pks + pks[:2]) == ([0, 1, 2, 3, 4, 0, 1], [rm.ADMITTED] * 5 + [rm.DUPLICATE] * 2)
    assert ctx.registry_level() == (5, 8)
    absent = hashlib.sha3_256(b"nobody").digest()
    assert ctx.registry_find(hs + [absent]) == [0, 1, 2, 3, 4, -1]
    coins = [rc.messages(k)[i] for i in idx]
    cts, sss, done = ctx.kem_enc_peers(hs, coins)
    want = rc.items(k)
    assert done == [True] * 5
    for b, i in enumerate(idx):
        assert kf.sha3(cts[b]) == want[i]["ct"] and sss[b].hex() == want[i]["ss"], (b, i)
    assert (cts, sss) == ctx.kem_enc(pks, coins)
    ids = (api.Kosk.PATH_REGISTRY_INDEX, api.Kosk.PATH_REGISTRY_FIND, api.Kosk.PATH_KEM_ENC_PEERS)
    before = tuple(ctx.path_count(i) for i in ids) + ctx.registry_level()
    assert before == (2, 3, 1, 5, 8)
    msg = _refused(lambda: ctx.registry_enrol_verified(3), "not available with call combining")
    assert "kosk_registry_enrol_verified" in msg and tuple(ctx.path_count(i) for i in ids) + ctx.registry_level() == before
    ctx.close()
    ctx = api.Kosk(kyber_k=k, max_batch=3, streams=2)
    ctx.registry_reserve(8)
    msg = _refused(lambda: ctx.registry_enrol_verified(3), "needs streams = 1")
    assert "kosk_registry_enrol_verified" in msg and ctx.registry_level() == (0, 8) and ctx.path_count(ids[0]) == 0
    ctx.close()
    print("cohort_member ok %d" % k)
