"""GPU tests of the relying party (include/kosk_mi355x.h: kosk_regtree_check_paths, kosk_regsort_check_proofs, kosk_kem_enc_proven;
INTEGRATION.md 8.9).  The ground truth is the host functions kosk_regtree_root_from_path and kosk_regsort_check_proof, which
tests/test_relying_host.py holds against the hashlib models on every table used here.  The checking handle has NO registry.  Every
comparison is exact."""
import ctypes as C
import hashlib
import os
import subprocess

import pytest

from tests import kem_fixture as kf
from tests import registry_cases as rc
from tests import registry_sorted_model as sm
from tests import relying_cases as cases

pytestmark = pytest.mark.gpu

KS = rc.KS
D = cases.D
SENTINEL = 0xA5
OLD_IDS = range(46)


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
def worlds(api):
    """per kyber_k, made at first use: a registrar handle holding the fixture registry with what it hands out, and a relying handle that
    holds nothing"""
    made = {}

    def world(k):
        if k not in made:
            reg = api.Kosk(kyber_k=k, max_batch=3)
            rc.admit_fixture(reg, k)
            slots = [rc.slot(i) for i in range(kf.ITEMS)]
            states, hs, paths, root = reg.registry_prove_slots(slots + cases.empty_slots(k))
            made[k] = {"reg": reg, "rel": api.Kosk(kyber_k=k, max_batch=1), "slots": slots, "states": states, "hs": hs, "paths": paths, "root": root,
                       "sroot": reg.registry_sorted_root()[0]}
        return made[k]
    yield world
    for w in made.values():
        w["reg"].close()
        w["rel"].close()


def ids(ctx, which=(46, 47, 48)):
    return tuple(ctx.path_count(i) for i in which)


def old_ids(ctx):
    return tuple(ctx.path_count(i) for i in OLD_IDS)


def host_path_ok(api, k, d, slot, state, h, path, root):
    got = C.create_string_buffer(32)
    r = api.lib.kosk_regtree_root_from_path(k, d, slot, C.c_char_p(h) if state else None, C.c_char_p(path) if d else None, got)
    return 1 if r == 0 and got.raw == root else 0


# ---- verdicts -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_path_verdicts(k, worlds, api):
    """1. the registrar's own paths of the 130 keys and of ten empty slots check on a handle without a registry; then every crafted table:
    item by item the host function's verdict.  One launch of k_regtree_check per call, ids 0..45 do not move"""
    w = worlds(k)
    rel = w["rel"]
    t = cases.path_table(k)
    assert w["root"] == t["root"] and w["states"] == [1] * 130 + [0] * 10
    assert rel.registry_level() == (0, 0)
    before, old = ids(rel), old_ids(rel)
    assert rel.regtree_check_paths(D, w["slots"] + cases.empty_slots(k), w["hs"], w["paths"], w["root"], states=w["states"]) == [1] * 140
    assert rel.regtree_check_paths(D, w["slots"], w["hs"][:130], w["paths"][:130], w["root"]) == [1] * 130  # states=None: all occupied
    calls = 2
    for t in cases.all_path_tables(api, k):
        slots, hs, paths, states = cases.path_args(t)
        want = cases.host_paths(api, t)
        got = rel.regtree_check_paths(t["depth"], slots, hs, paths, t["root"], states=states)
        for c, a, b in zip(t["cases"], got, want):
            assert a == b, (k, t["depth"], c[0], a, b)
        calls += 1
    # "empty" claims alone need no fingerprints
    e = cases.empty_slots(k)
    assert rel.regtree_check_paths(D, e, None, w["paths"][130:], w["root"], states=[0] * 10) == [1] * 10
    assert ids(rel) == (before[0] + calls + 1, before[1], before[2]) and old_ids(rel) == old and rel.registry_level() == (0, 0)


@pytest.mark.parametrize("k", KS)
def test_proof_verdicts(k, worlds, api):
    """2. the registrar's own records for every key, its neighbours, 00^32 and FF^32 check on a handle without a registry as what the
    registrar called them; then every crafted table, the 2 000 mutations among them: item by item the host function's verdict"""
    w = worlds(k)
    rel = w["rel"]
    t = cases.proof_table(k)
    assert w["sroot"] == t["root"]
    queries = [cases.ZERO, cases.ONES]
    for h in w["hs"][:130]:
        queries += [h] + sm.neighbours(h)
    kinds, records, root = w["reg"].registry_prove_absent(queries)
    assert root == t["root"]
    before, old = ids(rel), old_ids(rel)
    got = rel.regsort_check_proofs(D, queries, records, root)
    assert got == kinds == [api.regsort_check_proof(k, D, x, r, root) for x, r in zip(queries, records)]
    assert set(got) == {sm.ABSENT, sm.PRESENT}
    calls = 1
    for t in cases.all_proof_tables(k):
        want = cases.host_proofs(api, t)
        got = rel.regsort_check_proofs(t["depth"], [c[1] for c in t["cases"]], [c[2] for c in t["cases"]], t["root"])
        for c, a, b in zip(t["cases"], got, want):
            assert a == b, (k, t["depth"], c[0], a, b)
        calls += 1
    assert ids(rel) == (before[0], before[1] + calls, before[2]) and old_ids(rel) == old


def test_device_memory_and_odd_offsets(worlds, api, torch_cuda):
    """3. the crafted tables again, k = 3: every array in device memory at an odd byte offset between sentinel bytes, and in host memory at
    an odd offset: the same outputs as from lists"""
    torch = torch_cuda
    k = 3
    rel = worlds(k)["rel"]

    def dev(blob):
        return torch.frombuffer(bytearray(b"\x00" + blob), dtype=torch.uint8).cuda()

    def host(blob):
        buf = C.create_string_buffer(b"\x00" + blob, len(blob) + 1)
        return buf, C.addressof(buf) + 1
    t = cases.path_table(k)
    slots, hs, paths, states = cases.path_args(t)
    n = len(slots)
    want = rel.regtree_check_paths(D, slots, hs, paths, t["root"], states=states)
    assert want == cases.host_paths(api, t) and 0 in want and 1 in want
    blobs = [b"".join(s.to_bytes(4, "little", signed=True) for s in slots), b"".join(hs), b"".join(paths), bytes(states), t["root"]]
    d = [dev(b) for b in blobs]
    out = torch.full((1 + n + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rel.regtree_check_paths(D, d[0].data_ptr() + 1, d[1].data_ptr() + 1, d[2].data_ptr() + 1, d[4].data_ptr() + 1, states=d[3].data_ptr() + 1,
                            out=out.data_ptr() + 1, n=n)
    got = out.cpu().tolist()
    assert got[0] == SENTINEL and got[1:1 + n] == want and got[1 + n:] == [SENTINEL] * 8
    hbufs = [host(b) for b in blobs]
    res = C.create_string_buffer(bytes([SENTINEL]) * (n + 9), n + 9)
    rel.regtree_check_paths(D, hbufs[0][1], hbufs[1][1], hbufs[2][1], hbufs[4][1], states=hbufs[3][1], out=C.addressof(res) + 1, n=n)
    assert list(res.raw) == [SENTINEL] + want + [SENTINEL] * 8

    t = cases.proof_table(k)
    xs, recs = [c[1] for c in t["cases"]], [c[2] for c in t["cases"]]
    n = len(xs)
    want = rel.regsort_check_proofs(D, xs, recs, t["root"])
    assert want == cases.host_proofs(api, t) and set(want) == {0, 1, 2}
    blobs = [b"".join(xs), b"".join(recs), t["root"]]
    d = [dev(b) for b in blobs]
    out = torch.full((1 + n + 8,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rel.regsort_check_proofs(D, d[0].data_ptr() + 1, d[1].data_ptr() + 1, d[2].data_ptr() + 1, out=out.data_ptr() + 1, n=n)
    got = out.cpu().tolist()
    assert got[0] == SENTINEL and got[1:1 + n] == want and got[1 + n:] == [SENTINEL] * 8
    hbufs = [host(b) for b in blobs]
    res = C.create_string_buffer(bytes([SENTINEL]) * (n + 9), n + 9)
    rel.regsort_check_proofs(D, hbufs[0][1], hbufs[1][1], hbufs[2][1], out=C.addressof(res) + 1, n=n)
    assert list(res.raw) == [SENTINEL] + want + [SENTINEL] * 8


# ---- batch edges ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (1, 63, 64, 65, rc.CHUNK, rc.CHUNK + 1))
def test_batch_edges(n, worlds, api):
    """4. k = 2, items modulo the fixture with every 7th tampered, item 0 among them and item 16 384 not: a second launch group that
    wrapped around would answer for item 0.  Every item against the host function; ids 46 and 47 move by the number of launch groups,
    ids 0..45 not at all"""
    k = 2
    w = worlds(k)
    rel = w["rel"]
    groups = 1 if n <= rc.CHUNK else 2
    before, old = ids(rel), old_ids(rel)
    slots, hs, paths, want = [], [], [], []
    verdict = {}
    for b in range(n):
        i = b % kf.ITEMS
        bad = b % 7 == 0
        p = cases.flip(w["paths"][i], (b * 131) % (256 * D)) if bad else w["paths"][i]
        key = (i, (b * 131) % (256 * D) if bad else -1)
        if key not in verdict:
            verdict[key] = host_path_ok(api, k, D, w["slots"][i], 1, w["hs"][i], p, w["root"])
        slots.append(w["slots"][i]); hs.append(w["hs"][i]); paths.append(p); want.append(verdict[key])
    assert want == [0 if b % 7 == 0 else 1 for b in range(n)]
    assert rel.regtree_check_paths(D, slots, hs, paths, w["root"]) == want
    # proofs: PRESENT records of the fixture keys, every 7th with one byte changed in the part the verdict depends on
    t = cases.proof_table(k)
    pool = [(c[1], c[2]) for c in t["cases"] if c[0] == "PRESENT"]
    xs, recs, wantp = [], [], []
    verdict = {}
    for b in range(n):
        i = b % len(pool)
        x, rec = pool[i]
        at = 16 + (b * 37) % (32 + 0) if b % 7 == 0 else -1  # a byte of h_l
        if at >= 0:
            rec = rec[:at] + bytes([rec[at] ^ 0x80]) + rec[at + 1:]
        if (i, at) not in verdict:
            verdict[(i, at)] = api.regsort_check_proof(k, D, x, rec, t["root"])
        xs.append(x); recs.append(rec); wantp.append(verdict[(i, at)])
    assert wantp == [sm.NEITHER if b % 7 == 0 else sm.PRESENT for b in range(n)]
    assert rel.regsort_check_proofs(D, xs, recs, t["root"]) == wantp
    assert ids(rel) == (before[0] + groups, before[1] + groups, before[2]) and old_ids(rel) == old


# ---- kosk_kem_enc_proven --------------------------------------------------------------------------------------------------
def proven_items(k, w, n):
    """n items modulo the fixture: a tampered path at position 0, in the middle and at the last position, one pk with a flipped byte under
    its correct path; item 2 of the fixture (12-bit fields >= q, admitted as such) among the good ones"""
    idx = [b % kf.ITEMS for b in range(n)]
    pks = [rc.pks(k)[i] for i in idx]
    paths = [w["paths"][i] for i in idx]
    slots = [w["slots"][i] for i in idx]
    for b in (0, n // 2, n - 1):
        paths[b] = cases.flip(paths[b], (b * 53 + 7) % (256 * D))
    swapped = 5
    bad = bytearray(pks[swapped]); bad[100] ^= 1
    pks[swapped] = bytes(bad)
    return idx, pks, slots, paths, sorted({0, n // 2, n - 1, swapped})


@pytest.mark.parametrize("k", KS)
def test_kem_enc_proven(k, worlds, api):
    """5. 130 fixture keys with the registrar's paths and explicit coins: done is the host function's verdict on (slot, SHA3-256(pk as sent),
    path as sent); where it is 1, ct and ss are those of kosk_kem_enc_batch and of the reference's fixture, and the peers decapsulate;
    where it is 0 they are zero.  One launch of k_regtree_check and one encapsulation on id 48; ids 0..45 do not move"""
    w = worlds(k)
    rel = w["rel"]
    n = kf.ITEMS
    idx, pks, slots, paths, bad = proven_items(k, w, n)
    assert 2 not in bad
    coins = list(rc.messages(k))
    want_done = [bool(host_path_ok(api, k, D, slots[b], 1, hashlib.sha3_256(pks[b]).digest(), paths[b], w["root"])) for b in range(n)]
    assert want_done == [b not in bad for b in range(n)]
    plain = rel.kem_enc(pks, coins)
    before, old = ids(rel), old_ids(rel)
    cts, sss, done = rel.kem_enc_proven(D, pks, slots, paths, w["root"], coins)
    assert ids(rel) == (before[0] + 1, before[1], before[2] + 1) and old_ids(rel) == old
    assert done == want_done
    fixture = rc.items(k)
    for b in range(n):
        if done[b]:
            assert cts[b] == plain[0][b] and sss[b] == plain[1][b], b
            assert kf.sha3(cts[b]) == fixture[b]["ct"] and sss[b].hex() == fixture[b]["ss"], b
        else:
            assert cts[b] == bytes(kf.CT_BYTES[k]) and sss[b] == bytes(32), b
    # the peers' own secret keys; item 2's sk holds the canonical encoding of its pk, whose hash is another: it decapsulates to a rejection
    good = [b for b in range(n) if done[b] and b != 2]
    assert w["reg"].kem_dec([cts[b] for b in good], [kf.keypair(k, b)[1] for b in good]) == [sss[b] for b in good]
    # coins=None: one 32-byte draw per item, in item order; a refused call draws none
    calls = []

    def rb(nbytes):
        out = hashlib.shake_256(b"relying-callback:%d:%d" % (k, len(calls))).digest(nbytes)
        calls.append(out)
        return out
    rel.set_randombytes(rb)
    try:
        got = rel.kem_enc_proven(D, pks[:9], slots[:9], paths[:9], w["root"])
        assert [len(c) for c in calls] == [32] * 9
        assert got == rel.kem_enc_proven(D, pks[:9], slots[:9], paths[:9], w["root"], calls[:9]) and len(calls) == 9
        assert got[2] == want_done[:9] and got[0][1] == rel.kem_enc(pks[1:2], calls[1:2])[0][0]
        with pytest.raises(api.KoskError, match="kosk_kem_enc_proven: depth outside 0..31"):
            rel.kem_enc_proven(32, pks[:9], slots[:9], [bytes(32 * 32)] * 9, w["root"])
        assert len(calls) == 9
    finally:
        rel.set_randombytes(None)


def test_kem_enc_proven_two_launch_groups(worlds, api):
    """6. 16 385 items, k = 2: a tampered path at position 0, in the middle and at the last position, each held against the host function;
    ct and ss of every item against the per-item call on the same 16 385 items.  The second launch group is the last item alone (case 4
    holds the check kernel's second group against wrapping around).  Two launches on ids 46 and 48"""
    k = 2
    w = worlds(k)
    rel = w["rel"]
    n = rc.CHUNK + 1
    idx, pks, slots, paths, bad = proven_items(k, w, n)
    for b in bad:
        assert not host_path_ok(api, k, D, slots[b], 1, hashlib.sha3_256(pks[b]).digest(), paths[b], w["root"])
    msgs = rc.messages(k)
    coins = [msgs[i] for i in idx]
    ref = rel.kem_enc(pks, coins)  # the per-item call on the same items; it also grows the KEM workspace to a full launch group (id 18, as for every KEM call)
    before, old = ids(rel), old_ids(rel)
    cts, sss, done = rel.kem_enc_proven(D, pks, slots, paths, w["root"], coins)
    assert ids(rel) == (before[0] + 2, before[1], before[2] + 2) and old_ids(rel) == old
    assert done == [b not in bad for b in range(n)] and done[rc.CHUNK - 1] and not done[n - 1] and not done[0]
    zero_ct = bytes(kf.CT_BYTES[k])
    for b in range(n):
        if done[b]:
            assert cts[b] == ref[0][b] and sss[b] == ref[1][b], b
        else:
            assert cts[b] == zero_ct and sss[b] == bytes(32), b


# ---- isolation ------------------------------------------------------------------------------------------------------------
def test_isolation(worlds, api, oracle):
    """7. the three calls on a handle that verified earlier: kosk_kem_enc_verified returns what it returned before; the registrar's roots
    and its index are what they were"""
    k = 2
    w = worlds(k)
    reg = w["reg"]
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    pks, sks, pis = ctx.verifiable_keygen([oracle.tape_bytes_for(k, 60 + i) for i in range(3)])
    bad = bytearray(pis[1]); bad[1000] ^= 1
    assert ctx.verify([pis[0], bytes(bad), pis[2]], pks) == [True, False, True]
    coins = [hashlib.shake_256(b"relying-verified:%d" % i).digest(32) for i in range(3)]
    first = ctx.kem_enc_verified(3, coins)
    assert first[2] == [True, False, True]
    t = cases.proof_table(k)
    reg_state = (reg.registry_root(), reg.registry_sorted_root(), reg.registry_find(w["hs"][:5]), reg.path_count(api.Kosk.PATH_REGISTRY_INDEX))
    for handle in (ctx, reg):
        assert handle.regtree_check_paths(D, w["slots"][:7], w["hs"][:7], w["paths"][:7], w["root"]) == [1] * 7
        assert ctx.kem_enc_verified(3, coins) == first
        assert handle.regsort_check_proofs(D, [c[1] for c in t["cases"][:7]], [c[2] for c in t["cases"][:7]], t["root"]) == [sm.ABSENT] * 7
        assert ctx.kem_enc_verified(3, coins) == first
        assert handle.kem_enc_proven(D, list(rc.pks(k)[:7]), w["slots"][:7], w["paths"][:7], w["root"], list(rc.messages(k)[:7]))[2] == [True] * 7
        assert ctx.kem_enc_verified(3, coins) == first
    assert (reg.registry_root(), reg.registry_sorted_root(), reg.registry_find(w["hs"][:5]), reg.path_count(api.Kosk.PATH_REGISTRY_INDEX)) == reg_state
    ctx.close()


def test_inventory_and_erasure(worlds, api):
    """8. the staging buffers are public entries of the inventory from the first call on: a staged query fingerprint is found before
    kosk_wipe_secrets and after it; under KOSK_WIPE_CALL no coin of kosk_kem_enc_proven is left when it returns"""
    k = 2
    w = worlds(k)
    ctx = api.Kosk(kyber_k=k, max_batch=1)
    t = cases.proof_table(k)
    x = cases.fp(b"a staged query")
    assert ctx.secret_scan(x) == 0
    assert ctx.regsort_check_proofs(D, [x], [t["cases"][0][2]], t["root"]) == [api.regsort_check_proof(k, D, x, t["cases"][0][2], t["root"])]
    assert ctx.secret_scan(x) == 1
    ctx.wipe_secrets()
    assert ctx.secret_scan(x) == 1
    h = cases.fp(b"a staged fingerprint")
    assert ctx.regtree_check_paths(D, w["slots"][:1], [h], w["paths"][:1], w["root"]) == [0]
    assert ctx.secret_scan(h) == 1 and ctx.secret_scan(x) == 0  # the same buffer, the next call's item
    coin = hashlib.shake_256(b"relying-coin").digest(32)
    assert ctx.kem_enc_proven(D, [rc.pks(k)[0]], w["slots"][:1], w["paths"][:1], w["root"], [coin])[2] == [True]
    assert ctx.secret_scan(coin) >= 1
    ctx.set_wipe(api.WIPE_CALL)
    got = ctx.kem_enc_proven(D, [rc.pks(k)[0]], w["slots"][:1], w["paths"][:1], w["root"], [coin])
    assert got[2] == [True] and got[:2] == ctx.kem_enc([rc.pks(k)[0]], [coin])
    assert ctx.secret_scan(coin) == 0 and ctx.secret_scan(h) == 1
    ctx.set_wipe(api.WIPE_OFF)
    ctx.close()


# ---- refusals, the example, other handles ---------------------------------------------------------------------------------
def test_refusals(api):
    """9. each NULL, n = 0, depth = -1 and depth = 32: -1, a text that begins with the call's name, no path id moved"""
    k = 3
    ctx = api.Kosk(kyber_k=k, max_batch=1)
    lib, h = api.lib, ctx.handle
    buf = C.create_string_buffer(8192)
    slots = (C.c_int32 * 2)(0, 0)
    before = tuple(ctx.path_count(i) for i in range(49))

    def refused(rc_, name):
        assert rc_ == -1 and lib.kosk_last_error(h).startswith(name.encode() + b": "), (name, lib.kosk_last_error(h))
    paths_args = [h, 1, 1, slots, buf, buf, buf, buf, buf]
    for at in (3, 6, 7, 8):  # slots, paths (depth 1), root, ok
        a = list(paths_args); a[at] = None
        refused(lib.kosk_regtree_check_paths(*a), "kosk_regtree_check_paths")
    a = list(paths_args); a[4] = None; a[5] = None  # neither claims nor fingerprints
    refused(lib.kosk_regtree_check_paths(*a), "kosk_regtree_check_paths")
    proofs_args = [h, 1, 1, buf, buf, buf, buf]
    for at in (3, 4, 5, 6):
        a = list(proofs_args); a[at] = None
        refused(lib.kosk_regsort_check_proofs(*a), "kosk_regsort_check_proofs")
    proven_args = [h, 1, 1, buf, slots, buf, buf, buf, buf, buf, buf]
    for at in (3, 4, 5, 6, 8, 9, 10):  # pk, slots, paths (depth 1), root, ct, ss, done; coins may be NULL
        a = list(proven_args); a[at] = None
        refused(lib.kosk_kem_enc_proven(*a), "kosk_kem_enc_proven")
    for n, depth in ((0, 1), (-3, 1), (1, -1), (1, 32)):
        a = list(paths_args); a[1] = n; a[2] = depth
        refused(lib.kosk_regtree_check_paths(*a), "kosk_regtree_check_paths")
        a = list(proofs_args); a[1] = n; a[2] = depth
        refused(lib.kosk_regsort_check_proofs(*a), "kosk_regsort_check_proofs")
        a = list(proven_args); a[1] = n; a[2] = depth
        refused(lib.kosk_kem_enc_proven(*a), "kosk_kem_enc_proven")
    assert tuple(ctx.path_count(i) for i in range(49)) == before == (0,) * 49
    assert buf.raw == bytes(8192)
    # depth 0 needs no paths, "empty" claims no fingerprints
    e = api.regtree_leaf(k, None)
    assert ctx.regtree_check_paths(0, [0, 0, 1], None, None, e, states=[0, 0, 0]) == [1, 1, 0]
    ctx.close()


def test_cohort_member_in_a_child_process(gpu_child):
    """10. a cohort member, unmerged, in a fresh child process"""
    out = gpu_child("from tests.gpu_child_relying import cohort_member as f; f(2)")
    assert "cohort_member ok 2" in out


def test_registry_relying_example(torch_cuda):
    """11. examples/registry_relying 3 8 prints only lines ending in "= 1" """
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "registry_relying")
    if not os.path.exists(exe):
        pytest.fail("examples/registry_relying missing: run __graft_entry__.build()")
    r = subprocess.run([exe, "3", "8"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 8 and all(ln.endswith("= 1") for ln in lines), r.stdout
    assert lines[-1] == "[result] registry_relying success = 1"
