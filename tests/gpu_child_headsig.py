"""Child-process cases of tests/test_gpu_40_headsig.py (signed heads): a lowered per-launch leaf bound, and handles of
another kind than the module's."""
from tests import headsig_cases as hc


def many_launches():
    """KOSK_DEBUG_HEADSIG_LEAF_LAUNCH (set by the parent) bounds a leaf launch below the 2 048 leaves of height 11: the public key is the
    golden one whatever the number of launches, and height 5 still takes one"""
    import os
    from mpcith_kyber_kosk_amd import api
    bound = int(os.environ["KOSK_DEBUG_HEADSIG_LEAF_LAUNCH"])
    g = hc.golden()
    ctx = api.Kosk(kyber_k=hc.K, max_batch=1)
    ctx.registry_reserve(4)
    ctx.registry_history_reserve(4)
    assert ctx.registry_signer_reserve(11, hc.SEED, hc.ID).hex() == g["pub"]["h11"]
    launches = ctx.path_count(api.Kosk.PATH_HEADSIG_LEAVES)
    assert launches == (2048 + bound - 1) // bound and ctx.path_count(api.Kosk.PATH_HEADSIG_TREE) == 2
    assert ctx.registry_signer_reserve(5, hc.SEED, hc.ID) == hc.key(5).pub and ctx.path_count(api.Kosk.PATH_HEADSIG_LEAVES) == launches + 1
    ctx.close()
    print("many_launches ok %d" % launches)


def two_handles():
    """a cohort member is the registrar, unmerged; a second, plain handle without a registry verifies its heads on the GPU"""
    from mpcith_kyber_kosk_amd import api
    g = hc.golden()
    reg = api.Kosk(kyber_k=hc.K, max_batch=3, combine=2)
    reg.registry_reserve(hc.CAPACITY)
    reg.registry_history_reserve(40)
    pub = reg.registry_signer_reserve(hc.H_SIGN, hc.SEED, hc.ID)
    pks, heads = hc.history(hc.K, g["sign_tag"])
    reg.registry_admit(pks[:12], list(range(12)))
    sizes = [0, 1, 5, 12]
    signed = [reg.registry_history_sign_head(n) for n in sizes]
    assert [s[1] for s in signed] == [heads[n] for n in sizes]
    assert [s[0] for s in signed] == [hc.key(hc.H_SIGN).sign(hc.K, heads[n], n) for n in sizes]
    gate = api.Kosk(kyber_k=hc.K, max_batch=1)
    sigs = [s[0] for s in signed]
    roots = [s[1] for s in signed]
    assert gate.headsig_verify_heads(pub, roots, sizes, sigs) == [1, 1, 1, 1]
    assert gate.headsig_verify_heads(pub, roots[::-1], sizes, sigs) == [0, 0, 0, 0]
    assert reg.headsig_verify_heads(pub, roots, [0, 1, 5, 13], sigs) == [1, 1, 1, 0]
    assert (gate.path_count(52), reg.path_count(52), reg.path_count(51), gate.registry_level()) == (2, 1, 4, (0, 0))
    gate.close()
    reg.close()
    print("two_handles ok")
