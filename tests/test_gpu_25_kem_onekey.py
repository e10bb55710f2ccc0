"""GPU tests of the KEM with one resident key (include/kosk_mi355x.h: kosk_kem_key_set, kosk_kem_key_state, kosk_kem_key_clear,
kosk_kem_enc_key, kosk_kem_dec_key) against tests/golden/kem_onekey_v1.json -- what the reference's
crypto_kem_enc_derand / crypto_kem_dec returned for one key and many items -- and against the per-item calls on the same handle with the
record replicated.  Every comparison is exact.  Handles use max_batch = 3: the KEM calls do not depend on it."""
import ctypes as C
import hashlib
import os
import subprocess

import pytest

from tests import gpu_child_onekey as ok
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
def api(torch_cuda):
    from mpcith_kyber_kosk_amd import api
    return api


@pytest.fixture(scope="module")
def handles(api):
    hs = {k: api.Kosk(kyber_k=k, max_batch=3) for k in KS}
    yield hs
    for h in hs.values():
        h.close()


def _counts(ctx, api):
    ids = (api.Kosk.PATH_KEM_KEY_SETUP, api.Kosk.PATH_KEM_ENC_KEY, api.Kosk.PATH_KEM_DEC_KEY, 12, 13)
    return tuple(ctx.path_count(i) for i in ids)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k", KS)
def test_enc_and_dec_equal_the_reference(k, n, handles, api):
    """1. every position of kosk_kem_enc_key and kosk_kem_dec_key against the fixture (items modulo 130), the slot loaded from the pk
    (encapsulation) and again from the sk (both)"""
    ctx, v = handles[k], ok.vectors(k)
    ctx.kem_key_set(pk=v["pk"])
    assert ctx.kem_key_state() == api.KEM_KEY_PK
    ok.check_parity(ctx, k, n, False)
    ctx.kem_key_set(sk=v["sk"])
    assert ctx.kem_key_state() == api.KEM_KEY_SK
    ok.check_parity(ctx, k, n, True)


@pytest.mark.parametrize("k", KS)
def test_one_key_calls_equal_the_per_item_calls(k, handles, api):
    """2. on the same handle, for the canonical key, the non-canonical pk, the non-canonical s-hat and an sk whose stored H(pk) has one
    flipped bit: enc_key / dec_key == enc_batch / dec_batch with the record replicated, over more than a wave, one ciphertext tampered"""
    ctx, v = handles[k], ok.vectors(k)
    n = 67
    coins = [v["m"][b] for b in range(n)]
    bad_h = bytearray(v["sk"]); bad_h[-64] ^= 1
    valid_cts = None
    for name, sk in (("canonical", v["sk"]), ("nc_pk", v["nc_pk_sk"]), ("nc_shat", v["nc_shat_sk"]), ("bad_h", bytes(bad_h))):
        pk = sk[384 * k:384 * k + ctx.pk_bytes]
        ctx.kem_key_set(pk=pk)
        want = ctx.kem_enc([pk] * n, coins)
        assert ctx.kem_enc_key(coins=coins) == want, name
        ctx.kem_key_set(sk=sk)
        assert ctx.kem_enc_key(coins=coins) == want, name  # the pk inside the sk
        cts = list(want[0])
        cts[9] = kf.tampered(cts[9], kf.U_BYTES[k] - 1)
        got = ctx.kem_dec_key(cts)
        assert got == ctx.kem_dec(cts, [sk] * n), name
        assert got[9] == ok.rejection_key(sk, cts[9]), name
        if name == "canonical":
            valid_cts = want
            assert got[:9] == want[1][:9]
        if name == "nc_pk":
            assert [[kf.sha3(c), s.hex()] for c, s in zip(want[0][:8], want[1][:8])] == v["raw"]["nc_pk"] and got[:8] == want[1][:8]
        if name == "nc_shat":
            assert want == valid_cts and [g.hex() for g in got[:8]] == v["raw"]["nc_shat"]
        if name == "bad_h":  # decapsulation trusts the stored H(pk): G(m' || h') re-encrypts to another ciphertext, every item is rejected
            assert want == valid_cts and got == [ok.rejection_key(sk, c) for c in cts]


@pytest.mark.parametrize("k", KS)
def test_rejection_keys_alone_and_mixed(k, handles):
    """3. the three tampered ciphertexts of item 5 alone, together, and interleaved with valid ones over more than one wave (46 items):
    each position gets its own answer"""
    ctx, v = handles[k], ok.vectors(k)
    ctx.kem_key_set(sk=v["sk"])
    ct5 = bytes.fromhex(v["raw"]["ct5_hex"])
    bad = [kf.tampered(ct5, t["byte"]) for t in v["raw"]["tampered"]]
    want = [t["dec_ss"] for t in v["raw"]["tampered"]]
    assert [s.hex() for s in ctx.kem_dec_key(bad)] == want
    for b in range(3):
        assert ctx.kem_dec_key([bad[b]])[0].hex() == want[b]
    cts, _ = ctx.kem_enc_key(coins=[v["m"][i] for i in (0, 1, 3)])
    valid = [(cts[j], v["items"][i][1]) for j, i in enumerate((0, 1, 3))]
    mix = []
    for r in range(23):
        mix.append(valid[r % 3])
        mix.append((bad[(r // 3) % 3], want[(r // 3) % 3]))
    assert [s.hex() for s in ctx.kem_dec_key([x[0] for x in mix])] == [x[1] for x in mix]


def test_round_trip_on_device_buffers(handles, torch_cuda):
    """4. ct / ss / coins in device memory (torch), K = 3, n = 65, a sentinel around every output, nothing outside them written"""
    torch = torch_cuda
    k, n, pad = 3, 65, 64
    ctx, v = handles[k], ok.vectors(k)
    ctb = kf.CT_BYTES[k]
    coins = [v["m"][b] for b in range(n)]
    d_m = torch.frombuffer(bytearray(b"".join(coins)), dtype=torch.uint8).cuda()
    d_sk = torch.frombuffer(bytearray(v["sk"]), dtype=torch.uint8).cuda()
    d_ct = torch.full((pad + n * ctb + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_ss = torch.full((pad + n * 32 + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_ss2 = torch.full((pad + n * 32 + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.kem_key_set(sk=d_sk.data_ptr())  # the record itself in device memory
    ctx.kem_enc_key(n=n, coins=d_m.data_ptr(), out=(d_ct.data_ptr() + pad, d_ss.data_ptr() + pad))
    ctx.kem_dec_key(d_ct.data_ptr() + pad, n=n, out=d_ss2.data_ptr() + pad)
    ct, ss, ss2 = bytes(d_ct.cpu().numpy()), bytes(d_ss.cpu().numpy()), bytes(d_ss2.cpu().numpy())
    for buf in (ct, ss, ss2):
        assert buf[:pad] == bytes([SENTINEL]) * pad and buf[-pad:] == bytes([SENTINEL]) * pad
    assert ss == ss2
    for b in range(n):
        assert kf.sha3(ct[pad + ctb * b:pad + ctb * (b + 1)]) == v["items"][b][0] and ss[pad + 32 * b:pad + 32 * b + 32].hex() == v["items"][b][1]
    assert bytes(d_m.cpu().numpy()) == b"".join(coins) and bytes(d_sk.cpu().numpy()) == v["sk"]


@pytest.mark.parametrize("k", KS)
def test_coins_from_the_randombytes_callback(k, handles):
    """5. coins=None: exactly n calls of 32 bytes, in item order, and the results of the explicit-coins call on what the callback returned"""
    ctx, v = handles[k], ok.vectors(k)
    ctx.kem_key_set(pk=v["pk"])
    n = 7
    calls = []

    def rb(nbytes):
        out = hashlib.shake_256(b"kem-onekey-callback:%d:%d" % (k, len(calls))).digest(nbytes)
        calls.append(out)
        return out
    ctx.set_randombytes(rb)
    try:
        got = ctx.kem_enc_key(n=n)
    finally:
        ctx.set_randombytes(None)
    assert [len(c) for c in calls] == [32] * n
    assert got == ctx.kem_enc_key(coins=calls) == ctx.kem_enc([v["pk"]] * n, calls)
    assert len(calls) == n


@pytest.mark.parametrize("k", KS)
def test_state_machine_counters_and_neighbours(k, api, oracle):
    """6. the refusals with their texts and nothing started; the three new path ids; a second load replaces the key; the other calls of
    the handle around the new ones return what they return without them; a KEM workspace growth leaves the slot intact"""
    v = ok.vectors(k)
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    lib, h = api.lib, ctx.handle
    ctb = kf.CT_BYTES[k]
    buf = C.create_string_buffer(2 * ctb)
    ss = C.create_string_buffer(64)
    coins5 = v["m"][:5]
    # what the neighbours return before any key is loaded
    tapes = [oracle.tape_bytes_for(k, 30 + i) for i in range(3)]
    pks, sks, pis = ctx.verifiable_keygen(tapes)
    assert ctx.verify(pis, pks) == [True] * 3
    verified0 = ctx.kem_enc_verified(3, coins5[:3])
    enc0 = ctx.kem_enc([v["pk"]] * 5, coins5)
    dec0 = ctx.kem_dec(enc0[0], [v["sk"]] * 5)
    before = _counts(ctx, api)
    assert ctx.kem_key_state() == api.KEM_KEY_NONE
    with pytest.raises(api.KoskError, match="no key is loaded"):
        ctx.kem_enc_key(coins=coins5)
    with pytest.raises(api.KoskError, match="no key is loaded"):
        ctx.kem_dec_key(enc0[0])
    for args in ((h, None, None), (h, C.c_char_p(v["pk"]), C.c_char_p(v["sk"]))):  # neither, both
        assert lib.kosk_kem_key_set(*args) == -1 and b"kosk_kem_key_set: invalid argument" in lib.kosk_last_error(h)
    assert ctx.kem_key_state() == api.KEM_KEY_NONE and _counts(ctx, api) == before
    ctx.kem_key_set(pk=v["pk"])
    assert _counts(ctx, api) == (before[0] + 1,) + before[1:]  # one launch of k_kem_key_setup per load
    before = _counts(ctx, api)
    with pytest.raises(api.KoskError, match="public key"):
        ctx.kem_dec_key(enc0[0])
    for n in (0, -1):
        assert lib.kosk_kem_enc_key(h, n, None, buf, ss) == -1 and b"kosk_kem_enc_key: invalid argument" in lib.kosk_last_error(h)
        assert lib.kosk_kem_dec_key(h, n, buf, ss) == -1 and b"kosk_kem_dec_key: invalid argument" in lib.kosk_last_error(h)
    assert lib.kosk_kem_enc_key(h, 1, None, None, ss) == -1 and lib.kosk_kem_enc_key(h, 1, None, buf, None) == -1
    assert lib.kosk_kem_dec_key(h, 1, None, ss) == -1 and lib.kosk_kem_dec_key(h, 1, buf, None) == -1
    assert _counts(ctx, api) == before
    ctx.kem_key_set(sk=v["sk"])
    assert ctx.kem_enc_key(coins=coins5) == enc0 and ctx.kem_dec_key(enc0[0]) == dec0
    big = ctx.kem_enc_key(coins=[v["m"][b % kf.ITEMS] for b in range(CHUNK + 1)])  # two launch groups
    assert CHUNK % kf.ITEMS == 4 and big[0][CHUNK] == enc0[0][4] and big[1][CHUNK] == enc0[1][4] and big[1][:5] == enc0[1]
    assert _counts(ctx, api) == (before[0] + 1, before[1] + 3, before[2] + 1, before[3], before[4])  # ids 12 / 13 do not move
    # a second load replaces the key
    pk4, sk4 = kf.keypair(k, 4)
    ctx.kem_key_set(sk=sk4)
    enc4 = ctx.kem_enc_key(coins=coins5)
    assert enc4 == ctx.kem_enc([pk4] * 5, coins5) and enc4 != enc0
    assert ctx.kem_dec_key(enc4[0]) == enc4[1] and ctx.kem_dec_key(enc0[0]) == ctx.kem_dec(enc0[0], [sk4] * 5)
    ctx.kem_key_set(sk=v["sk"])
    # the neighbours with a key loaded: the same answers
    assert ctx.kem_enc_verified(3, coins5[:3]) == verified0
    assert ctx.kem_enc([v["pk"]] * 5, coins5) == enc0 and ctx.kem_dec(enc0[0], [v["sk"]] * 5) == dec0
    assert tuple(ctx.verifiable_keygen(tapes)) == (pks, sks, pis) and ctx.verify(pis, pks) == [True] * 3
    opk, osk, opi, _, _ = oracle.verifiable_keygen(k, tapes[0])
    assert (pks[0], sks[0], pis[0]) == (opk, osk, opi)
    assert ctx.kem_enc_key(coins=coins5) == enc0 and ctx.kem_dec_key(enc0[0]) == dec0
    ctx.close()
    # a workspace growth (a per-item call of 1025 items after a small one) frees and reallocates the workspace, not the slot
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    ctx.kem_key_set(sk=v["sk"])
    assert ctx.kem_enc([v["pk"]] * 5, coins5) == enc0
    grown = ctx.kem_enc([v["pk"]] * 1025, [v["m"][b % kf.ITEMS] for b in range(1025)])
    assert grown[0][:5] == enc0[0] and kf.sha3(grown[0][1024]) == v["items"][1024 % kf.ITEMS][0]
    assert ctx.kem_key_state() == api.KEM_KEY_SK
    assert ctx.kem_enc_key(coins=coins5) == enc0 and ctx.kem_dec_key(enc0[0]) == dec0
    ctx.close()


@pytest.mark.parametrize("k", KS)
def test_wiping(k, api):
    """7. z of the loaded key and a decapsulated ss as needles"""
    v = ok.vectors(k)
    z = v["sk"][-32:]
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    assert ctx.secret_scan(z) == 0
    ctx.kem_key_set(sk=v["sk"])
    assert ctx.secret_scan(z) >= 1
    enc0 = ctx.kem_enc_key(coins=v["m"][:3])
    ss0 = ctx.kem_dec_key(enc0[0])
    assert ss0 == enc0[1] and ctx.secret_scan(ss0[1]) >= 1  # mode off: the scratch keeps it
    ctx.wipe_secrets()
    assert ctx.secret_scan(z) == 0 and ctx.secret_scan(ss0[1]) == 0
    assert ctx.kem_key_state() == api.KEM_KEY_PK
    assert ctx.kem_enc_key(coins=v["m"][:3]) == enc0
    with pytest.raises(api.KoskError, match="wiped"):
        ctx.kem_dec_key(enc0[0])
    # KOSK_WIPE_CALL: the slot is a long-lived secret; the wipe at the end of a call clears the scratch and leaves it alone
    ctx.set_wipe(api.WIPE_CALL)
    ctx.kem_key_set(sk=v["sk"])
    assert ctx.kem_key_state() == api.KEM_KEY_SK
    hits = ctx.secret_scan(z)
    assert hits >= 1
    assert ctx.kem_dec_key(enc0[0]) == ss0
    assert ctx.secret_scan(z) == hits and ctx.secret_scan(ss0[1]) == 0
    assert ctx.kem_enc_key(coins=v["m"][:3]) == enc0 and ctx.secret_scan(ss0[1]) == 0 and ctx.secret_scan(z) == hits
    assert ctx.kem_dec_key(enc0[0]) == ss0
    ctx.set_wipe(api.WIPE_OFF)
    ctx.kem_key_clear()
    assert ctx.secret_scan(z) == 0 and ctx.kem_key_state() == api.KEM_KEY_NONE
    with pytest.raises(api.KoskError, match="no key is loaded"):
        ctx.kem_dec_key(enc0[0])
    ctx.close()


def test_per_lane_rkprf_on_small_batches(torch_cuda, gpu_child):
    """8. KOSK_DEBUG_KEM_WAVE_MAX=0: the per-lane rkprf on n = 3 and 65 against the fixture"""
    out = gpu_child("from tests.gpu_child_onekey import per_lane_rkprf_on_small_batches as f; f(2); f(3); f(4)",
                    env={"KOSK_DEBUG_KEM_WAVE_MAX": "0"})
    for k in KS:
        assert "per_lane_rkprf_on_small_batches ok %d" % k in out


def test_both_paths_on_one_handle(torch_cuda, gpu_child):
    """10. the slot's pointers and the workspace's under the shared kernels: per-item calls on 65 keys that are not the slot's and
    one-key calls on 65 items, alternating twice on one handle, every ct and ss against its fixture, one rejected ciphertext in the second
    wave of each dec; again with KOSK_DEBUG_KEM_WAVE_MAX=0 (H(pk) and rkprf on the per-lane roles)"""
    ok.both_paths_on_one_handle(3)
    out = gpu_child("from tests.gpu_child_onekey import both_paths_on_one_handle as f; f(3)", env={"KOSK_DEBUG_KEM_WAVE_MAX": "0"})
    assert "both_paths_on_one_handle ok 3" in out


def test_block_limit_inside_key_set(torch_cuda, gpu_child):
    """6. -1 ("block limit") with the slot left empty when gen_matrix reaches its limit inside kosk_kem_key_set"""
    out = gpu_child("from tests.gpu_child_onekey import block_limit_leaves_the_slot_empty as f; f(3)", env={"KOSK_DEBUG_XOF_BLOCKS": "1"})
    assert "block_limit_leaves_the_slot_empty ok 3" in out


def test_cohort_member_uses_the_calls_unmerged(torch_cuda, gpu_child):
    out = gpu_child("from tests.gpu_child_onekey import cohort_member_uses_the_calls_unmerged as f; f(2)")
    assert "cohort_member_uses_the_calls_unmerged ok 2" in out


def test_kem_onekey_example(torch_cuda):
    """9. examples/kem_onekey 3 8 prints only lines ending in "= 1" """
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "kem_onekey")
    if not os.path.exists(exe):
        pytest.fail("examples/kem_onekey missing: run __graft_entry__.build()")
    r = subprocess.run([exe, "3", "8"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 8 and all(ln.endswith("= 1") for ln in lines), r.stdout
    assert lines[-1] == "[result] kem_onekey success = 1"
