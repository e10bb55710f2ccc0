"""Shared pieces and child-process cases of tests/test_gpu_25_kem_onekey.py (KEM with one resident key)."""
import functools
import hashlib
import importlib.util
import json
import os

from tests import kem_fixture as kf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = 3  # the fixture's key: kf.keypair(k, 3)


@functools.lru_cache(maxsize=None)
def generator():
    spec = importlib.util.spec_from_file_location("make_kem_onekey_vectors", os.path.join(ROOT, "tests", "golden", "make_kem_onekey_vectors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@functools.lru_cache(maxsize=None)
def vectors(k):
    """the fixture of one K with its regenerated inputs -- computed once, never modified"""
    with open(os.path.join(ROOT, "tests", "golden", "kem_onekey_v1.json")) as f:
        v = json.load(f)["k"]["k%d" % k]
    gen = generator()
    pk, sk = kf.keypair(k, KEY)
    pk2, sk2 = gen.nc_pk_sk(k)
    return {"raw": v, "items": gen.items_of(v), "pk": pk, "sk": sk, "m": [kf.message(k, i) for i in range(kf.ITEMS)],
            "nc_pk": pk2, "nc_pk_sk": sk2, "nc_shat_sk": gen.nc_shat_sk(k)}


def check_parity(ctx, k, n, dec):
    """n items (fixture items modulo 130) through kosk_kem_enc_key and, with dec, kosk_kem_dec_key: every position against the fixture"""
    v = vectors(k)
    idx = [b % kf.ITEMS for b in range(n)]
    cts, sss = ctx.kem_enc_key(coins=[v["m"][i] for i in idx])
    assert len(cts) == n and len(sss) == n
    for b, i in enumerate(idx):
        assert kf.sha3(cts[b]) == v["items"][i][0], ("ct", k, n, b)
        assert sss[b].hex() == v["items"][i][1], ("ss", k, n, b)
    if dec:
        got = ctx.kem_dec_key(cts)
        for b, i in enumerate(idx):
            assert got[b].hex() == v["items"][i][1], ("dec", k, n, b)
        assert kf.sha3(b"".join(got[:kf.ITEMS])) == v["raw"]["dec"] or n < kf.ITEMS
    return cts, sss


def per_lane_rkprf_on_small_batches(k=3):
    """run with KOSK_DEBUG_KEM_WAVE_MAX=0: the rkprf of small batches on the per-lane role of k_kem_key_hash (what batches above
    KEM_WAVE_MAX use), against the fixture, valid and tampered ciphertexts"""
    assert os.environ.get("KOSK_DEBUG_KEM_WAVE_MAX") == "0"
    from mpcith_kyber_kosk_amd import api
    v = vectors(k)
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.kem_key_set(sk=v["sk"])
    for n in (3, 65):
        check_parity(ctx, k, n, True)
    ct5 = bytes.fromhex(v["raw"]["ct5_hex"])
    bad = [kf.tampered(ct5, t["byte"]) for t in v["raw"]["tampered"]]
    assert [s.hex() for s in ctx.kem_dec_key(bad)] == [t["dec_ss"] for t in v["raw"]["tampered"]]
    ctx.close()
    print("per_lane_rkprf_on_small_batches ok %d" % k)


def cohort_member_uses_the_calls_unmerged(k=2):
    from mpcith_kyber_kosk_amd import api
    v = vectors(k)
    ctx = api.Kosk(kyber_k=k, max_batch=3, combine=2)
    ctx.kem_key_set(sk=v["sk"])
    assert ctx.kem_key_state() == api.KEM_KEY_SK
    cts, sss = check_parity(ctx, k, 5, True)
    assert (cts, sss) == ctx.kem_enc([v["pk"]] * 5, v["m"][:5])
    assert ctx.path_count(api.Kosk.PATH_KEM_ENC_KEY) == 1 and ctx.path_count(api.Kosk.PATH_KEM_DEC_KEY) == 1
    ctx.kem_key_clear()
    assert ctx.kem_key_state() == api.KEM_KEY_NONE
    ctx.close()
    print("cohort_member_uses_the_calls_unmerged ok %d" % k)


def block_limit_leaves_the_slot_empty(k=3):
    """run with KOSK_DEBUG_XOF_BLOCKS=1: gen_matrix reaches its block limit inside kosk_kem_key_set -- -1 "block limit", the slot empty,
    also when it replaces nothing and when the handle is used afterwards"""
    assert os.environ.get("KOSK_DEBUG_XOF_BLOCKS") == "1"
    from mpcith_kyber_kosk_amd import api
    v = vectors(k)
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    for kw in ({"sk": v["sk"]}, {"pk": v["pk"]}):
        try:
            ctx.kem_key_set(**kw)
        except api.KoskError as e:
            assert "block limit" in str(e), str(e)
        else:
            raise AssertionError("kosk_kem_key_set did not report the block limit")
        assert ctx.kem_key_state() == api.KEM_KEY_NONE and ctx.secret_scan(v["sk"][-32:]) == 0
        try:
            ctx.kem_enc_key(coins=v["m"][:1])
        except api.KoskError as e:
            assert "no key is loaded" in str(e), str(e)
        else:
            raise AssertionError("kosk_kem_enc_key on the empty slot did not fail")
    assert ctx.path_count(api.Kosk.PATH_KEM_KEY_SETUP) == 2 and ctx.path_count(api.Kosk.PATH_KEM_ENC_KEY) == 0
    ctx.close()
    print("block_limit_leaves_the_slot_empty ok %d" % k)


def rejection_key(sk, ct):
    return hashlib.shake_256(sk[-32:] + ct).digest(32)
