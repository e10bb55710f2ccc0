"""GPU tests of signed heads (include/kosk_mi355x.h: kosk_registry_signer_reserve / _level, kosk_registry_history_sign_head,
kosk_headsig_verify_heads; INTEGRATION.md 8.10, format kosk-headsig-v1) against the hashlib model of tests/headsig_model.py, the golden
file and the host function kosk_headsig_verify.  Every comparison is exact.  Shapes: heights 1, 2 and 5 leave the leaf kernel's blocks
ragged at both ends of the 7 items a block, 10 is exactly one tree tier, 11 two tiers; batches sit on the edges of 7."""
import ctypes as C
import hashlib
import os
import struct
import subprocess

import pytest

from tests import headsig_cases as hc
from tests import headsig_model as m

pytestmark = pytest.mark.gpu

SENTINEL = 0xA5
IPB = 7  # KOSK_HEADSIG_ITEMS_PER_BLOCK
NEW_IDS = (49, 50, 51, 52)


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return torch


@pytest.fixture(scope="module")
def api(torch_cuda):
    from mpcith_kyber_kosk_amd import api
    assert api.HEADSIG_ITEMS_PER_BLOCK == IPB
    return api


@pytest.fixture(scope="module")
def golden():
    return hc.golden()


def new_ids(ctx):
    return tuple(ctx.path_count(i) for i in NEW_IDS)


def old_ids(ctx):
    return tuple(ctx.path_count(i) for i in range(49))


def registrar(api, golden, height=hc.H_SIGN, max_events=40, events=True):
    """a handle with a registry of 32 slots, a history, a signer of `height` and (events) the 31 admissions of headsig_cases.history"""
    ctx = api.Kosk(kyber_k=hc.K, max_batch=1)
    ctx.registry_reserve(hc.CAPACITY)
    ctx.registry_history_reserve(max_events)
    pub = ctx.registry_signer_reserve(height, hc.SEED, hc.ID)
    if events:
        pks, _ = hc.history(hc.K, golden["sign_tag"])
        ctx.registry_admit(pks, list(range(len(pks))))
    return ctx, pub


def refused(api, ctx, rc_, name, word=None):
    text = api.lib.kosk_last_error(ctx.handle)
    assert rc_ == -1 and text.startswith(name.encode() + b": ") and (word is None or word.encode() in text), (name, text)


# ---- key generation ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h", (1, 2, 5, 10, 11))
def test_public_key_against_the_golden_file(h, api, golden):
    """1. the leaf kernel and the tree's tiers: 2, 4 and 32 leaves are one ragged block and five blocks with a ragged last one; 1 024
    leaves are one tier exactly, 2 048 two blocks of tier 0 and an upper tier"""
    ctx = api.Kosk(kyber_k=hc.K, max_batch=1)
    ctx.registry_reserve(4)
    ctx.registry_history_reserve(4)
    assert ctx.registry_signer_level() == (0, False) and new_ids(ctx) == (0, 0, 0, 0)
    before = old_ids(ctx)
    pub = ctx.registry_signer_reserve(h, hc.SEED, hc.ID)
    assert pub.hex() == golden["pub"]["h%d" % h]
    assert ctx.registry_signer_level() == (h, True)
    assert new_ids(ctx) == (1, (h + 9) // 10, 0, 0) and old_ids(ctx) == before
    if h <= 5:
        assert pub == hc.key(h).pub and pub != ctx.registry_signer_reserve(h, hc.OTHER_SEED, hc.ID) == hc.key(h, hc.OTHER_SEED).pub
    ctx.registry_signer_reserve(0)
    assert ctx.registry_signer_level() == (0, False)
    ctx.close()


def test_every_leaf_and_node_of_height_5(api, golden):
    """2. the 32 signatures' paths hold every node but the root, the public key holds the root: all 63 against the model"""
    ctx, pub = registrar(api, golden)
    key = hc.key(5)
    seen = {1: pub[20:]}
    for q in range(32):
        sig, _, _ = ctx.registry_history_sign_head(q)
        for l in range(5):
            seen[((32 + q) >> l) ^ 1] = sig[1136 + 32 * l:1168 + 32 * l]
    assert sorted(seen) == list(range(1, 64))
    for r, node in seen.items():
        assert node == key.T[r], r
    ctx.close()


def test_many_leaf_launches_in_a_child_process(gpu_child, golden):
    """3. the per-launch leaf bound lowered to 701 (no multiple of 7): height 11 takes three leaf launches with ragged last blocks"""
    out = gpu_child("from tests.gpu_child_headsig import many_launches as f; f()", env={"KOSK_DEBUG_HEADSIG_LEAF_LAUNCH": "701"})
    assert "many_launches ok 3" in out


# ---- signing ----------------------------------------------------------------------------------------------------------------
def test_every_size_is_signed_as_the_model_signs_it(api, golden):
    """4. a history of 31 events at height 5: sizes 0..31, byte for byte, among them a chain of no steps and one of all 255"""
    ctx, pub = registrar(api, golden)
    _, heads = hc.history(hc.K, golden["sign_tag"])
    want, seen = hc.history_signatures(hc.K, golden["sign_tag"])
    assert 0 in seen and 255 in seen
    assert hashlib.sha3_256(b"".join(want)).hexdigest() == golden["history_signatures_sha3_256"]
    before, frontier = old_ids(ctx), ctx.path_count(40)
    for n in range(32):
        sig, root, size = ctx.registry_history_sign_head(n)
        assert (root, size) == (heads[n], n) and sig == want[n], n
        assert api.headsig_verify(pub, hc.K, root, n, sig) is True
        assert api.headsig_verify(pub, 3, root, n, sig) is False
    assert ctx.registry_history_sign_head() == (want[31], heads[31], 31)
    assert ctx.registry_history_sign_head(17) == ctx.registry_history_sign_head(17) == (want[17], heads[17], 17)  # one size, one record
    after = old_ids(ctx)
    assert new_ids(ctx) == (1, 1, 35, 0)
    assert after[:40] + after[41:] == before[:40] + before[41:] and after[40] > frontier  # only the frontier's id moves
    # the signer is exhausted at 2^h, and a size above the current one is no size
    lib, h_ = api.lib, ctx.handle
    buf, root = C.create_string_buffer(api.headsig_sig_bytes(5)), C.create_string_buffer(32)
    refused(api, ctx, lib.kosk_registry_history_sign_head(h_, 32, buf, root, None), "kosk_registry_history_sign_head", "above the current size")
    ctx.registry_evict([0])  # event 31: the history has 32 events now
    refused(api, ctx, lib.kosk_registry_history_sign_head(h_, 32, buf, root, None), "kosk_registry_history_sign_head", "signer is exhausted")
    refused(api, ctx, lib.kosk_registry_history_sign_head(h_, -1, buf, root, None), "kosk_registry_history_sign_head", "signer is exhausted")
    refused(api, ctx, lib.kosk_registry_history_sign_head(h_, 33, buf, root, None), "kosk_registry_history_sign_head", "above the current size")
    refused(api, ctx, lib.kosk_registry_history_sign_head(h_, 5, None, root, None), "kosk_registry_history_sign_head", "null pointer")
    assert buf.raw == bytes(len(buf.raw)) and root.raw == bytes(32) and new_ids(ctx) == (1, 1, 35, 0)
    assert ctx.registry_history_sign_head(31) == (want[31], heads[31], 31)
    ctx.close()


def test_device_outputs_at_odd_alignment(api, golden, torch_cuda):
    """5. pub, sig and root into device memory one byte past an allocation; seed and id out of device memory at odd addresses"""
    torch = torch_cuda
    ctx = api.Kosk(kyber_k=hc.K, max_batch=1)
    ctx.registry_reserve(hc.CAPACITY)
    ctx.registry_history_reserve(40)
    d_seed = torch.frombuffer(bytearray(b"\x00" + hc.SEED), dtype=torch.uint8).cuda()
    d_id = torch.frombuffer(bytearray(b"\x00\x00\x00" + hc.ID), dtype=torch.uint8).cuda()
    d_pub = torch.full((1 + 52 + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.registry_signer_reserve(5, d_seed.data_ptr() + 1, d_id.data_ptr() + 3, out=d_pub.data_ptr() + 1)
    got = bytes(d_pub.cpu().tolist())
    assert got[0] == SENTINEL and got[1:53] == hc.key(5).pub and got[53:] == bytes([SENTINEL]) * 8
    pks, heads = hc.history(hc.K, golden["sign_tag"])
    ctx.registry_admit(pks[:9], list(range(9)))
    sb = api.headsig_sig_bytes(5)
    d_sig = torch.full((3 + sb + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_root = torch.full((1 + 32 + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert ctx.registry_history_sign_head(9, out=(d_sig.data_ptr() + 3, d_root.data_ptr() + 1))[2] == 9
    sig, root = bytes(d_sig.cpu().tolist()), bytes(d_root.cpu().tolist())
    assert sig[:3] == bytes([SENTINEL]) * 3 and sig[3 + sb:] == bytes([SENTINEL]) * 8 and root[0] == SENTINEL and root[33:] == bytes([SENTINEL]) * 8
    assert root[1:33] == heads[9] and sig[3:3 + sb] == hc.key(5).sign(hc.K, heads[9], 9)
    ctx.close()


def test_wipe_refuses_signing_and_a_reserve_restores_the_seed(api, golden):
    """6. kosk_wipe_secrets zeroes the seed: signing is refused, the tree and the key stay; the same seed comes back without a build,
    another seed is another key; under KOSK_WIPE_CALL the seed stays.  The scan finds the seed before the wipe and not after, and never
    an x_q[i] of a signed leaf"""
    ctx, pub = registrar(api, golden)
    _, heads = hc.history(hc.K, golden["sign_tag"])
    want = hc.key(5).sign(hc.K, heads[20], 20)
    assert ctx.registry_history_sign_head(20)[0] == want
    assert ctx.secret_scan(hc.SEED) == 1
    for i in (0, 33):
        assert ctx.secret_scan(m.x_start(hc.ID, 20, i, hc.SEED)) == 0
    assert ctx.secret_scan(want[16:48]) >= 1  # the staged signature is a public entry: the scan covers it
    ctx.set_wipe(api.WIPE_CALL)
    ctx.kem_enc([hc.event_key(hc.K, 0, 0)], [bytes(32)])  # a call that ends with the per-call wipe
    assert ctx.registry_signer_level() == (5, True) and ctx.secret_scan(hc.SEED) == 1 and ctx.registry_history_sign_head(20)[0] == want
    ctx.set_wipe(api.WIPE_OFF)
    ctx.wipe_secrets()
    assert ctx.registry_signer_level() == (5, False) and ctx.secret_scan(hc.SEED) == 0
    counts = new_ids(ctx)
    buf, root = C.create_string_buffer(api.headsig_sig_bytes(5)), C.create_string_buffer(32)
    refused(api, ctx, api.lib.kosk_registry_history_sign_head(ctx.handle, 20, buf, root, None), "kosk_registry_history_sign_head", "seed was wiped")
    assert buf.raw == bytes(len(buf.raw)) and new_ids(ctx) == counts
    assert ctx.registry_signer_reserve(5, hc.SEED, hc.ID) == pub  # leaf 0 from the seed against the standing tree: one launch, no tree
    assert new_ids(ctx) == (counts[0] + 1, counts[1], counts[2], 0) and ctx.registry_signer_level() == (5, True)
    assert ctx.registry_history_sign_head(20)[0] == want and ctx.secret_scan(hc.SEED) == 1
    other = ctx.registry_signer_reserve(5, hc.OTHER_SEED, hc.ID)  # another seed under the same identifier: a new key, built whole
    assert other == hc.key(5, hc.OTHER_SEED).pub != pub and new_ids(ctx)[:2] == (counts[0] + 3, counts[1] + 1)
    sig = ctx.registry_history_sign_head(20)[0]
    assert sig == hc.key(5, hc.OTHER_SEED).sign(hc.K, heads[20], 20) and not api.headsig_verify(pub, hc.K, heads[20], 20, sig)
    assert ctx.secret_scan(hc.SEED) == 0 and ctx.secret_scan(hc.OTHER_SEED) == 1
    ctx.close()


def test_the_signer_goes_with_the_history_and_the_registry(api, golden):
    """7. freeing the history or the registry frees the signer; refusals name the call and start nothing"""
    ctx, pub = registrar(api, golden, height=2, events=False)
    assert ctx.registry_signer_level() == (2, True)
    ctx.registry_history_reserve(0)
    assert ctx.registry_signer_level() == (0, False) and ctx.secret_scan(hc.SEED) == 0
    lib, h_ = api.lib, ctx.handle
    buf = C.create_string_buffer(2048)
    refused(api, ctx, lib.kosk_registry_signer_reserve(h_, 2, hc.SEED, hc.ID, buf), "kosk_registry_signer_reserve", "no history")
    refused(api, ctx, lib.kosk_registry_history_sign_head(h_, 0, buf, buf, None), "kosk_registry_history_sign_head", "no history")
    ctx.registry_history_reserve(8)
    refused(api, ctx, lib.kosk_registry_history_sign_head(h_, 0, buf, buf, None), "kosk_registry_history_sign_head", "no signer")
    for height in (-1, 25):
        refused(api, ctx, lib.kosk_registry_signer_reserve(h_, height, hc.SEED, hc.ID, buf), "kosk_registry_signer_reserve", "height")
    for at in (2, 3, 4):
        a = [h_, 2, hc.SEED, hc.ID, buf]
        a[at] = None
        refused(api, ctx, lib.kosk_registry_signer_reserve(*a), "kosk_registry_signer_reserve", "null pointer")
    assert buf.raw == bytes(2048) and new_ids(ctx) == (1, 1, 0, 0)
    assert ctx.registry_signer_reserve(2, hc.SEED, hc.ID) == pub == hc.key(2).pub
    sig, root, size = ctx.registry_history_sign_head()
    assert size == 0 and root == api.reghist_empty_root(hc.K) and sig == hc.key(2).sign(hc.K, root, 0)
    ctx.registry_reserve(0)
    assert ctx.registry_signer_level() == (0, False) and ctx.secret_scan(hc.SEED) == 0
    refused(api, ctx, lib.kosk_registry_signer_reserve(h_, 2, hc.SEED, hc.ID, buf), "kosk_registry_signer_reserve", "no registry")
    ctx.close()


# ---- batch verification -----------------------------------------------------------------------------------------------------
def mixed_batch(api, golden, n):
    """n items under key(5): valid ones, and from n = 3 on a tamper at the first, the middle and the last position"""
    roots, sizes, sigs, seen = hc.batch_items(hc.K, golden["batch_tag"], n)
    roots, sizes, sigs = list(roots), list(sizes), list(sigs)
    pub = hc.key(5).pub
    if n >= 3:
        t = m.tampers(5)
        for at, (name, f) in zip((0, n // 2, n - 1), (t[1], t[6], t[10])):  # z[0], the top of the path, q != size
            p2, roots[at], sizes[at], sigs[at] = f(pub, roots[at], sizes[at], sigs[at])
            assert p2 == pub, name
    return pub, roots, sizes, sigs, seen


def host_verdicts(api, pub, roots, sizes, sigs):
    return [int(api.headsig_verify(pub, hc.K, r, s, g)) for r, s, g in zip(roots, sizes, sigs)]


@pytest.fixture(scope="module")
def verifier(api):
    ctx = api.Kosk(kyber_k=hc.K, max_batch=1)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("n", (1, IPB - 1, IPB, IPB + 1, 2 * IPB + 1))
def test_batches_on_the_edges_of_a_block(n, api, golden, verifier):
    """8. one item, one short of a block, a block, one more, and one past two blocks, on a handle with no registry; every item is
    compared with the host function"""
    pub, roots, sizes, sigs, seen = mixed_batch(api, golden, n)
    want = host_verdicts(api, pub, roots, sizes, sigs)
    assert len(want) == n and want.count(0) == (3 if n >= 3 else 0)
    if n == 2 * IPB + 1:
        assert 0 in seen and 255 in seen  # a chain of all 255 steps and one of none among the items
    before, new = old_ids(verifier), new_ids(verifier)
    assert verifier.headsig_verify_heads(pub, roots, sizes, sigs) == want
    assert old_ids(verifier) == before and new_ids(verifier) == (0, 0, 0, new[3] + 1)
    assert verifier.registry_level() == (0, 0) and verifier.registry_signer_level() == (0, False)


def test_every_tamper_at_the_first_a_middle_and_the_last_position(api, golden, verifier):
    """9. each tamper of the host list as the sole defect of items 0, 7 and 14 of 15; a public key tamper fails every item"""
    n = 2 * IPB + 1
    roots, sizes, sigs, _ = hc.batch_items(hc.K, golden["batch_tag"], n)
    pub = hc.key(5).pub
    assert verifier.headsig_verify_heads(pub, roots, sizes, sigs) == [1] * n
    for name, f in m.tampers(5):
        r2, s2, g2, p2 = list(roots), list(sizes), list(sigs), pub
        for at in (0, IPB, n - 1):
            p2, r2[at], s2[at], g2[at] = f(pub, roots[at], sizes[at], sigs[at])
        want = host_verdicts(api, p2, r2, s2, g2)
        assert want == ([0] * n if p2 != pub else [0 if b in (0, IPB, n - 1) else 1 for b in range(n)]), name
        assert verifier.headsig_verify_heads(p2, r2, s2, g2) == want, name
    forged = m.advance_forgery(pub, hc.K, roots[3], sizes[3], sigs[3], 4)
    assert verifier.headsig_verify_heads(pub, roots, sizes, sigs[:3] + [forged] + sigs[4:]) == [1, 1, 1, 0] + [1] * (n - 4)
    # negative and huge sizes are peer data: a verdict, never a refusal
    assert verifier.headsig_verify_heads(pub, roots[:3], [-1, sizes[1], 0x7FFFFFFF], sigs[:3]) == [0, 1, 0]


def test_device_arrays_at_odd_alignment_and_two_launch_groups(api, golden, verifier, torch_cuda):
    """10. every array in device memory one byte past an allocation; 16 385 items are two launch groups"""
    torch = torch_cuda
    n = 16385
    pub, roots, sizes, sigs, _ = mixed_batch(api, golden, 2 * IPB + 1)
    want15 = host_verdicts(api, pub, roots, sizes, sigs)
    reps = (n + 14) // 15
    blobs = [b"".join(roots) * reps, struct.pack("<15i", *sizes) * reps, b"".join(sigs) * reps]
    d = [torch.frombuffer(bytearray(b"\x00" + b), dtype=torch.uint8).cuda() for b in blobs]
    out = torch.full((1 + n + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = new_ids(verifier)
    verifier.headsig_verify_heads(pub, d[0].data_ptr() + 1, d[1].data_ptr() + 1, d[2].data_ptr() + 1, out=out.data_ptr() + 1, n=n)
    got = out.cpu().tolist()
    assert got[0] == SENTINEL and got[1 + n:] == [SENTINEL] * 8
    assert got[1:1 + n] == (want15 * reps)[:n]
    assert new_ids(verifier) == (0, 0, 0, before[3] + 2)


def test_verifier_refusals(api, golden, verifier):
    """11. a NULL, n < 1 and a bad height in the public key are refusals that start nothing"""
    lib, h_ = api.lib, verifier.handle
    pub = hc.key(1).pub
    buf = C.create_string_buffer(4096)
    sizes = (C.c_int32 * 1)(0)
    before = new_ids(verifier)
    args = [h_, 1, pub, buf, sizes, buf, buf]
    for at in (2, 3, 4, 5, 6):
        a = list(args)
        a[at] = None
        refused(api, verifier, lib.kosk_headsig_verify_heads(*a), "kosk_headsig_verify_heads", "null pointer")
    for n in (0, -2):
        a = list(args)
        a[1] = n
        refused(api, verifier, lib.kosk_headsig_verify_heads(*a), "kosk_headsig_verify_heads", "n must be")
    for h in (0, 25, 0x80000000):
        a = list(args)
        a[2] = struct.pack("<I", h) + pub[4:]
        refused(api, verifier, lib.kosk_headsig_verify_heads(*a), "kosk_headsig_verify_heads", "height")
    assert buf.raw == bytes(4096) and new_ids(verifier) == before


def test_a_cohort_member_in_a_child_process(gpu_child):
    """12. a cohort member signs and verifies, unmerged, in a fresh child process; a second handle there verifies the first one's heads"""
    out = gpu_child("from tests.gpu_child_headsig import two_handles as f; f()")
    assert "two_handles ok" in out


def test_registry_signed_example(torch_cuda):
    """13. examples/registry_signed prints only lines ending in "= 1" """
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "registry_signed")
    if not os.path.exists(exe):
        pytest.fail("examples/registry_signed missing: run __graft_entry__.build()")
    r = subprocess.run([exe, "3", "8"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) >= 8 and all(ln.endswith("= 1") for ln in lines), r.stdout
    assert lines[-1] == "[result] registry_signed success = 1"
