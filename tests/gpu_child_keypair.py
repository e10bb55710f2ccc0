"""Child-process bodies of tests/test_gpu_20_kem_keypair.py (run through the gpu_child fixture with an environment of their own)."""
from tests import kem_keypair_cases as kk


def per_lane_hpk_on_small_batches(k):
    """with KOSK_DEBUG_KEM_WAVE_MAX=0 in the environment: H(pk) of the key pairs and of the sk checks runs one lane per item
    (k_kem_hpk hashing itself) at batch sizes where the wave sponge would otherwise serve.  pk_bytes / 8 = 100 / 148 / 196 words: 5, 8,
    11 full blocks of 17 with 15, 12, 9 words left."""
    from mpcith_kyber_kosk_amd import api
    ctx = api.Kosk(kyber_k=k, max_batch=1)
    try:
        for n in (1, 7, 70):
            want = [kk.keypair(k, i) for i in range(n)]
            pks, sks = ctx.kem_keypair([kk.coins(k, i) for i in range(n)])
            assert pks == [w[0] for w in want] and sks == [w[1] for w in want], (k, n)
            recs = list(sks)
            recs[n - 1] = kk.flip(recs[n - 1], len(recs[0]) - 64)          # first byte of the stored H(pk)
            recs[0] = kk.flip(recs[0], 384 * k + 5) if n > 1 else recs[0]   # a byte of the embedded pk
            want_flags = [kk.flags_sk(k, r) for r in recs]
            assert want_flags[n - 1] & kk.HASH and (n == 1 or want_flags[0] & kk.HASH)
            assert ctx.kem_check_sk(recs) == want_flags, (k, n)
            assert ctx.kem_check_sk(sks) == [0] * n
        assert ctx.path_count(api.Kosk.PATH_KEM_KEYPAIR) == 3 and ctx.path_count(api.Kosk.PATH_KEM_CHECK) == 6
    finally:
        ctx.close()
    print("per_lane_hpk_on_small_batches ok %d" % k)
