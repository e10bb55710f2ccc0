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
    """run with KOSK_DEBUG_KEM_WAVE_MAX=0: the rkprf of small batches on the per-lane role of k_kem_hash, z at stride 0 (what batches
    above KEM_WAVE_MAX use), against the fixture, valid and tampered ciphertexts"""
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


def both_paths_on_one_handle(k=3, n=65):
    """the per-item and the one-key calls share their kernels and their host bodies: with fixture key 3 in the slot, twice over,
    kosk_kem_enc_batch + kosk_kem_dec_batch on n items of tests/golden/kem_vectors_v1.json (each its own key, none of them key 3), then
    kosk_kem_enc_key + kosk_kem_dec_key on n items -- every ct and ss against its fixture.  65 items: a second, partial wave in every role.
    Rejected in the per-item dec: item 2 (the fixture stores its rejection key) and a tampered ciphertext in the second wave
    (SHAKE256(z || ct) of that item's own z); in the one-key dec: the fixture's tampered ciphertext of item 5, put in the second wave"""
    from mpcith_kyber_kosk_amd import api
    v, items = vectors(k), kf.load()["k"]["k%d" % k]
    idx = [i for i in range(n + 1) if i != KEY]
    pks, sks, ms = [kf.enc_pk(k, i) for i in idx], [kf.keypair(k, i)[1] for i in idx], [kf.message(k, i) for i in idx]
    t = v["raw"]["tampered"][1]
    bad5 = kf.tampered(bytes.fromhex(v["raw"]["ct5_hex"]), t["byte"])
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.kem_key_set(sk=v["sk"])
    for _ in range(2):
        cts, sss = ctx.kem_enc(pks, ms)
        assert [kf.sha3(c) for c in cts] == [items[i]["ct"] for i in idx] and [s.hex() for s in sss] == [items[i]["ss"] for i in idx]
        cts[n - 1] = kf.tampered(cts[n - 1], kf.U_BYTES[k] - 1)
        want = [items[i]["dec_ss"] if i == 2 else items[i]["ss"] for i in idx]
        want[n - 1] = rejection_key(sks[n - 1], cts[n - 1]).hex()
        assert [s.hex() for s in ctx.kem_dec(cts, sks)] == want
        cts, sss = check_parity(ctx, k, n, False)
        cts[n - 1] = bad5
        assert [s.hex() for s in ctx.kem_dec_key(cts)] == [x[1] for x in v["items"][:n - 1]] + [t["dec_ss"]]
    assert ctx.path_count(api.Kosk.PATH_KEM_ENC_KEY) == 2 and ctx.path_count(api.Kosk.PATH_KEM_DEC_KEY) == 2
    ctx.close()
    print("both_paths_on_one_handle ok %d" % k)


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
