"""Child-process case of tests/test_gpu_14_kem.py (a cohort handle lives in a fresh process, like every multi-handle case)."""


def enc_verified_refused_in_a_cohort(k=2):
    from mpcith_kyber_kosk_amd import api
    from tests import kem_fixture as kf
    ctx = api.Kosk(kyber_k=k, max_batch=3, combine=2)
    try:
        ctx.kem_enc_verified(1, coins=[bytes(32)])
    except api.KoskError as e:
        assert "call combining" in str(e), str(e)
    else:
        raise AssertionError("kosk_kem_enc_verified on a cohort member did not fail")
    # the two batch calls are not merged calls: they work on a member's own stream
    pk, sk = kf.keypair(k, 5)
    cts, sss = ctx.kem_enc([pk], [kf.message(k, 5)])
    it = kf.load()["k"]["k%d" % k][5]
    assert kf.sha3(cts[0]) == it["ct"] and sss[0].hex() == it["ss"]
    assert ctx.kem_dec(cts, [sk]) == sss
    ctx.close()
    print("enc_verified_refused_in_a_cohort ok %d" % k)


def per_lane_sponges_on_small_batches(k=3):
    """run with KOSK_DEBUG_KEM_WAVE_MAX=0: H(pk) and rkprf of small batches on the per-lane roles of k_kem_hash (what batches above
    KEM_WAVE_MAX use), against the fixture; and kosk_kem_enc_verified on that path, where the resident pk records are pk_stride apart"""
    import os
    assert os.environ.get("KOSK_DEBUG_KEM_WAVE_MAX") == "0"
    from mpcith_kyber_kosk_amd import api
    from tests import kem_fixture as kf
    from tests import oracle_lib
    items = kf.load()["k"]["k%d" % k]
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    idx = list(range(7))
    cts, sss = ctx.kem_enc([kf.enc_pk(k, i) for i in idx], [kf.message(k, i) for i in idx])
    assert [kf.sha3(c) for c in cts] == [items[i]["ct"] for i in idx] and [s.hex() for s in sss] == [items[i]["ss"] for i in idx]
    got = ctx.kem_dec(cts, [kf.keypair(k, i)[1] for i in idx])
    assert [g.hex() for g in got] == [items[i]["dec_ss"] if i == 2 else items[i]["ss"] for i in idx]
    ct3 = bytes.fromhex(items[3]["ct_hex"])
    for t in items[3]["tampered"]:
        assert ctx.kem_dec([kf.tampered(ct3, t["byte"])], [kf.keypair(k, 3)[1]])[0].hex() == t["dec_ss"]
    pks, sks, pis = ctx.verifiable_keygen([oracle_lib.tape_bytes_for(k, i) for i in range(3)])
    assert ctx.verify(pis, pks) == [True] * 3
    coins = [kf.message(k, 20 + i) for i in range(3)]
    cts, sss, done = ctx.kem_enc_verified(3, coins)
    assert done == [True] * 3 and (cts, sss) == ctx.kem_enc(pks, coins)
    assert ctx.kem_dec(cts, sks) == sss
    ctx.close()
    print("per_lane_sponges_on_small_batches ok %d" % k)
