"""GPU tests of the Kyber KEM calls (include/kosk_mi355x.h: kosk_kem_enc_batch, kosk_kem_dec_batch, kosk_kem_enc_verified) against
tests/golden/kem_vectors_v1.json -- what the reference's crypto_kem_enc_derand / crypto_kem_dec returned -- and against hashlib for
the rejection keys.  Every comparison is exact.  One handle per parameter set, max_batch = 3: the KEM calls do not depend on it."""
import hashlib
import os
import subprocess

import pytest

from tests import kem_fixture as kf

pytestmark = pytest.mark.gpu

KS = (2, 3, 4)
CHUNK = 16384  # KEM_CHUNK of csrc/kosk_ctx.hpp: items per launch group
SIZES = (1, 3, 65, 130, CHUNK + 1)  # one item, a partial wave, one past a wave, one past two, one past a launch group
SENTINEL = 0xA5


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return torch


@pytest.fixture(scope="module")
def handles(torch_cuda):
    from mpcith_kyber_kosk_amd import api
    hs = {k: api.Kosk(kyber_k=k, max_batch=3) for k in KS}
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope="module")
def vectors():
    """per K: the fixture's items with their regenerated keys and inputs -- computed once, never modified"""
    out = {}
    for k in KS:
        items = kf.load()["k"]["k%d" % k]
        keys = [kf.keypair(k, i) for i in range(kf.ITEMS)]
        for i, it in enumerate(items):
            assert kf.sha3(keys[i][0]) == it["pk"] and kf.sha3(keys[i][1]) == it["sk"]
        out[k] = {"items": items, "pk": [kf.enc_pk(k, i) for i in range(kf.ITEMS)], "sk": [s for _, s in keys],
                  "m": [kf.message(k, i) for i in range(kf.ITEMS)]}
    return out


def _check_enc(k, v, cts, sss, n):
    for b in range(n):
        it = v["items"][b % kf.ITEMS]
        if "ct_hex" in it and cts[b].hex() != it["ct_hex"]:
            want = bytes.fromhex(it["ct_hex"])
            at = next(j for j in range(len(want)) if want[j] != cts[b][j])
            pytest.fail("K=%d n=%d position %d (item %d): first differing ct byte %d: %02x, expected %02x"
                        % (k, n, b, b % kf.ITEMS, at, cts[b][at], want[at]))
        assert kf.sha3(cts[b]) == it["ct"], (k, n, b)
        assert sss[b].hex() == it["ss"], (k, n, b)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k", KS)
def test_enc_and_dec_equal_the_reference(k, n, handles, vectors):
    """enc: ct and ss of every position equal the fixture (items 0-2 included: m all zero, m all ones, a non-canonical pk encoding).
    dec of those ciphertexts under the canonical secret keys: ss again, except item 2, whose ciphertext was made for another encoding
    of the pk than the one in the sk: the stored rejection key."""
    ctx, v = handles[k], vectors[k]
    idx = [b % kf.ITEMS for b in range(n)]
    cts, sss = ctx.kem_enc([v["pk"][i] for i in idx], [v["m"][i] for i in idx])
    _check_enc(k, v, cts, sss, n)
    got = ctx.kem_dec(cts, [v["sk"][i] for i in idx])
    for b, i in enumerate(idx):
        want = v["items"][i]["dec_ss"] if i == 2 else v["items"][i]["ss"]
        assert got[b].hex() == want, (k, n, b)


@pytest.mark.parametrize("k", KS)
def test_dec_rejection_keys_and_mixed_batches(k, handles, vectors):
    """the three tampered ciphertexts of item 3 and item 2's ciphertext give the stored rejection keys = SHAKE256(z || ct); in one
    batch with valid items every position gets its own answer"""
    ctx, v = handles[k], vectors[k]
    items = v["items"]
    ct3, sk3 = bytes.fromhex(items[3]["ct_hex"]), v["sk"][3]
    cts, sks, want = [], [], []
    for t in items[3]["tampered"]:
        bad = kf.tampered(ct3, t["byte"])
        assert t["dec_ss"] == hashlib.shake_256(sk3[-32:] + bad).digest(32).hex()
        cts.append(bad); sks.append(sk3); want.append(t["dec_ss"])
    ct2 = bytes.fromhex(items[2]["ct_hex"])
    assert items[2]["dec_ss"] == hashlib.shake_256(v["sk"][2][-32:] + ct2).digest(32).hex()
    cts.append(ct2); sks.append(v["sk"][2]); want.append(items[2]["dec_ss"])
    assert [s.hex() for s in ctx.kem_dec(cts, sks)] == want
    for b in range(len(cts)):  # each alone
        assert ctx.kem_dec([cts[b]], [sks[b]])[0].hex() == want[b]
    # mixed: valid, tampered, valid, tampered ... over more than one wave of items
    valid = [(bytes.fromhex(items[i]["ct_hex"]), v["sk"][i], items[i]["ss"]) for i in (0, 1, 3)]
    mix = []
    for r in range(23):
        mix.append(valid[r % 3])
        mix.append((cts[r % 4], sks[r % 4], want[r % 4]))
    assert [s.hex() for s in ctx.kem_dec([x[0] for x in mix], [x[1] for x in mix])] == [x[2] for x in mix]


def test_round_trip_on_device_buffers(handles, torch_cuda):
    """no reference: keys from verifiable_keygen on the same handle, random coins, dec(enc) == ss; every input and output a device
    buffer (torch), K = 3, n = 65, a sentinel around every output"""
    torch = torch_cuda
    k, n, pad = 3, 65, 64
    ctx = handles[k]
    ctb = kf.CT_BYTES[k]
    pks, sks, _ = ctx.verifiable_keygen(n=3)
    pks = [pks[b % 3] for b in range(n)]; sks = [sks[b % 3] for b in range(n)]
    coins = [os.urandom(32) for _ in range(n)]
    dev = lambda blobs: torch.frombuffer(bytearray(b"".join(blobs)), dtype=torch.uint8).cuda()
    d_pk, d_sk, d_m = dev(pks), dev(sks), dev(coins)
    d_ct = torch.full((pad + n * ctb + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_ss = torch.full((pad + n * 32 + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_ss2 = torch.full((pad + n * 32 + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.kem_enc(d_pk.data_ptr(), d_m.data_ptr(), n=n, out=(d_ct.data_ptr() + pad, d_ss.data_ptr() + pad))
    ctx.kem_dec(d_ct.data_ptr() + pad, d_sk.data_ptr(), n=n, out=d_ss2.data_ptr() + pad)
    ct, ss, ss2 = bytes(d_ct.cpu().numpy()), bytes(d_ss.cpu().numpy()), bytes(d_ss2.cpu().numpy())
    for buf in (ct, ss, ss2):
        assert buf[:pad] == bytes([SENTINEL]) * pad and buf[-pad:] == bytes([SENTINEL]) * pad
    assert ss == ss2 and len(set(ss[pad + 32 * b:pad + 32 * b + 32] for b in range(n))) == n
    # the same inputs as host buffers give the same bytes
    cts, sss = ctx.kem_enc(pks, coins)
    assert b"".join(cts) == ct[pad:-pad] and b"".join(sss) == ss[pad:-pad]
    # ss = first half of G(m || H(pk)) (kem.c:88-94), from hashlib
    for b in (0, 1, 64):
        assert sss[b] == hashlib.sha3_512(coins[b] + hashlib.sha3_256(pks[b]).digest()).digest()[:32]


@pytest.mark.parametrize("k", KS)
def test_coins_from_the_randombytes_callback(k, handles, vectors):
    """coins=None: exactly n calls of 32 bytes, in item order, and the results of the explicit-coins call on what the callback returned"""
    ctx, v = handles[k], vectors[k]
    n = 7
    calls = []

    def rb(nbytes):
        out = hashlib.shake_256(b"kem-callback:%d:%d" % (k, len(calls))).digest(nbytes)
        calls.append(out)
        return out
    ctx.set_randombytes(rb)
    try:
        got = ctx.kem_enc(v["pk"][10:10 + n])
    finally:
        ctx.set_randombytes(None)
    assert [len(c) for c in calls] == [32] * n
    assert got == ctx.kem_enc(v["pk"][10:10 + n], calls)
    assert len(calls) == n


def test_enc_verified(torch_cuda, oracle):
    from mpcith_kyber_kosk_amd import api
    k = 2
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    coins = [hashlib.shake_256(b"kem-verified:%d" % i).digest(32) for i in range(3)]
    with pytest.raises(api.KoskError, match="no verify call"):
        ctx.kem_enc_verified(3, coins)
    pks, sks, pis = ctx.verifiable_keygen([oracle.tape_bytes_for(k, i) for i in range(3)])
    with pytest.raises(api.KoskError, match="no verify call"):
        ctx.kem_enc_verified(3, coins)
    bad = bytearray(pis[1]); bad[1000] ^= 1
    ctx.stage_verifier_inputs([pis[0], bytes(bad), pis[2]], pks)
    assert ctx.verify_resident(3) == [True, False, True]
    cts, sss, done = ctx.kem_enc_verified(3, coins)
    assert done == [True, False, True]
    want_ct, want_ss = ctx.kem_enc(pks, coins)
    assert (cts[0], sss[0], cts[2], sss[2]) == (want_ct[0], want_ss[0], want_ct[2], want_ss[2])
    assert cts[1] == bytes(kf.CT_BYTES[k]) and sss[1] == bytes(32)
    assert ctx.kem_dec([cts[0], cts[2]], [sks[0], sks[2]]) == [sss[0], sss[2]]
    # coins drawn for every position, accepted or not
    calls = []

    def rb(nbytes):
        calls.append(nbytes)
        return coins[len(calls) - 1][:nbytes]
    ctx.set_randombytes(rb)
    try:
        assert ctx.kem_enc_verified(3) == (cts, sss, done) and calls == [32, 32, 32]
    finally:
        ctx.set_randombytes(None)
    # a verify call of fewer proofs than asked for
    ctx.stage_verifier_inputs(pis[:2], pks[:2])
    assert ctx.verify_resident(2) == [True, True]
    with pytest.raises(api.KoskError, match="fewer than n"):
        ctx.kem_enc_verified(3, coins)
    assert ctx.kem_enc_verified(2, coins[:2])[2] == [True, True]
    # a chunked kosk_verify_batch call (n > max_batch) leaves only its last chunk's keys
    assert ctx.verify(pis + pis[:1], pks + pks[:1]) == [True] * 4
    with pytest.raises(api.KoskError, match="chunked"):
        ctx.kem_enc_verified(2, coins[:2])
    ctx.close()


def test_enc_verified_refused_in_a_cohort(torch_cuda, gpu_child):
    out = gpu_child("from tests.gpu_child_kem import enc_verified_refused_in_a_cohort; enc_verified_refused_in_a_cohort(2)")
    assert "enc_verified_refused_in_a_cohort ok 2" in out


@pytest.mark.parametrize("k", KS)
def test_path_counts_and_the_pipeline_after_kem_calls(k, handles, vectors, oracle):
    """kem_enc / kem_dec count launch groups and nothing else moves; afterwards a verifiable_keygen + verify on the same handle still
    equals the oracle (the KEM workspace aliases nothing of the pipeline's)"""
    ctx, v = handles[k], vectors[k]
    before = ctx.path_counts()
    cts, sss = ctx.kem_enc(v["pk"][:5], v["m"][:5])
    ctx.kem_dec(cts, v["sk"][:5])
    ctx.kem_dec(cts[:1], v["sk"][:1])
    after = ctx.path_counts()
    assert after["kem_enc"] == before["kem_enc"] + 1 and after["kem_dec"] == before["kem_dec"] + 2
    assert {n: c for n, c in after.items() if not n.startswith("kem_")} == {n: c for n, c in before.items() if not n.startswith("kem_")}
    tape = oracle.tape_bytes_for(k, 1)
    pks, sks, pis = ctx.verifiable_keygen([tape])
    opk, osk, opi, _, _ = oracle.verifiable_keygen(k, tape)
    assert (pks[0], sks[0], pis[0]) == (opk, osk, opi)
    assert ctx.verify(pis, pks) == [True]
    # and the key it just proved is one the KEM calls can use
    ct, ss = ctx.kem_enc(pks, [v["m"][7]])
    assert ctx.kem_dec(ct, sks) == ss


@pytest.mark.parametrize("k", KS)
def test_kem_roundtrip_example(k, torch_cuda):
    """examples/kem_roundtrip.cpp on the C ABI: keygen, verify (proof 1 damaged), kosk_kem_enc_verified, kosk_kem_dec_batch, equal
    secrets; for K = 3 also the source-compatible crypto_kem_* face of include/kosk_compat.hpp"""
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "kem_roundtrip")
    if not os.path.exists(exe):
        pytest.fail("examples/kem_roundtrip missing: run __graft_entry__.build()")
    r = subprocess.run([exe, str(k), "5"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    assert "[kem] kyber_k %d: 5 proofs, 4 accepted, 4 shared secrets agree" % k in r.stdout
    assert "[kem] launch groups: enc 1 dec 1" in r.stdout and "[result] kem roundtrip success" in r.stdout
    assert ("[compat] crypto_kem_enc / crypto_kem_enc_derand / crypto_kem_dec agree = 1" in r.stdout) == (k == 3)


def _inst(api, k, seed64):
    """the mlwe_inst image (A, t, s, e) of kyber_keygen on seed64"""
    import ctypes as C
    import numpy as np
    pk = C.create_string_buffer(api.pk_bytes(k)); sk = C.create_string_buffer(api.sk_bytes(k))
    A = np.zeros(k * k * 256, np.int16); s = np.zeros(k * 256, np.int16); e = np.zeros(k * 256, np.int16); t = np.zeros(k * 256, np.int16)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert api.lib.kosk_keygen(k, seed64, pk, sk, vp(A), vp(s), vp(e), vp(t)) == 0
    return A.tobytes() + t.tobytes() + s.tobytes() + e.tobytes()


def test_enc_verified_refuses_keys_that_are_not_the_verified_ones(torch_cuda, oracle):
    """kosk_kem_enc_verified encapsulates only to the very key bytes the last verify call decoded: -1 after any call that replaced the
    resident keys (a verifier staging call, its compact form, a key generation), and -1 when the verifier's A and t came from
    instances (kosk_verify_inst) while older key bytes are still resident"""
    from mpcith_kyber_kosk_amd import api
    k = 2
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    tapes_a = [oracle.tape_bytes_for(k, 50 + i) for i in range(3)]
    tapes_b = [oracle.tape_bytes_for(k, 60 + i) for i in range(3)]
    pks_b, _, pis_b = ctx.verifiable_keygen(tapes_b)
    comp_b = ctx.verifiable_keygen_compact(tapes_b)[2]
    pks_a, sks_a, pis_a = ctx.verifiable_keygen(tapes_a)
    assert pks_a != pks_b
    coins = [hashlib.shake_256(b"kem-replaced:%d" % i).digest(32) for i in range(3)]

    def verify_a():
        ctx.stage_verifier_inputs(pis_a, pks_a)
        assert ctx.verify_resident(3) == [True] * 3
        cts, sss, done = ctx.kem_enc_verified(3, coins)
        assert done == [True] * 3 and (cts, sss) == ctx.kem_enc(pks_a, coins)
    verify_a()
    ctx.stage_verifier_inputs(pis_b, pks_b)
    with pytest.raises(api.KoskError, match="replaced"):
        ctx.kem_enc_verified(3, coins)
    verify_a()
    ctx.stage_verifier_inputs_compact(comp_b, pks_b)
    with pytest.raises(api.KoskError, match="replaced"):
        ctx.kem_enc_verified(3, coins)
    verify_a()
    ctx.verifiable_keygen(tapes_b[:1])
    with pytest.raises(api.KoskError, match="replaced"):
        ctx.kem_enc_verified(3, coins)
    verify_a()
    assert ctx.verify(pis_b, pks_b) == [True] * 3  # a whole verify call of other keys: those are the verified ones now
    cts, sss, done = ctx.kem_enc_verified(3, coins)
    assert done == [True] * 3 and (cts, sss) == ctx.kem_enc(pks_b, coins)
    # instances: keys A resident from a key generation, proofs B verified against their instances, then the resident verify call
    ctx.verifiable_keygen(tapes_a)
    assert ctx.verify_inst(pis_b, [_inst(api, k, t[:64]) for t in tapes_b]) == [True] * 3
    with pytest.raises(api.KoskError, match="no public key bytes"):
        ctx.kem_enc_verified(3, coins)
    assert ctx.verify_resident(3) == [True] * 3
    with pytest.raises(api.KoskError, match="no public key bytes"):
        ctx.kem_enc_verified(3, coins)
    # a resident-key verify call of FEWER proofs decodes only its own records: record 2 of the verifier's A and t is still instance B2,
    # so a following kosk_verify_resident(3) accepts proof B2 -- which never verified under resident key A2
    assert ctx.verify_resident_pk(2) == [False, False]
    assert ctx.verify_resident(3)[2] is True
    with pytest.raises(api.KoskError, match="no public key bytes"):
        ctx.kem_enc_verified(3, coins)
    # the resident keys decoded again by a verify call are verified keys: proofs B do not verify under keys A, nothing is encapsulated
    assert ctx.verify_resident_pk(3) == [False] * 3
    cts, sss, done = ctx.kem_enc_verified(3, coins)
    assert done == [False] * 3 and cts == [bytes(kf.CT_BYTES[k])] * 3 and sss == [bytes(32)] * 3
    verify_a()
    ctx.close()


def test_per_lane_sponges_on_small_batches(torch_cuda, gpu_child):
    """K = 2, 3, 4: the per-lane rkprf absorbs 4 + CT_BYTES / 8 = 100 / 140 / 200 words, i.e. 5, 8, 11 full blocks of 17 with 15, 4,
    13 words left, at a batch size (7) where its wave also holds lanes of the next role"""
    out = gpu_child("from tests.gpu_child_kem import per_lane_sponges_on_small_batches as f; f(2); f(3); f(4)",
                    env={"KOSK_DEBUG_KEM_WAVE_MAX": "0"})
    assert "per_lane_sponges_on_small_batches ok 3" in out
    assert "per_lane_sponges_on_small_batches ok 2" in out and "per_lane_sponges_on_small_batches ok 4" in out
