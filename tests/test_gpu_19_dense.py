"""GPU tests of the dense wire format kosk-dense-v1 (csrc/kosk_dense.hip: k_dense_setup, k_dense_fill, and the dense
field plan of the pack / unpack kernels in csrc/kosk_compact.hip).  References: the numpy model tests/dense_model.py for the refill and
the host codec (pinned to that model by tests/test_dense_host.py) for whole records.  Every comparison is exact."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests import dense_model as dm

pytestmark = pytest.mark.gpu

KS = (2, 3, 4)
GUARD = 256


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return t


def _api():
    from mpcith_kyber_kosk_amd import api
    return api


def _first_diff(a, b):
    d = np.nonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8))[0]
    return None if len(d) == 0 else (int(d[0]), len(d))


# ---- kernel level: kosk_dense_fill_device against the model
def _opened_sets(rng):
    third = list(range(0, 3 * dm.NOPEN, 3))
    rand = rng.permutation(dm.NPARTY)[:dm.NOPEN].tolist()
    dup = rng.permutation(dm.NPARTY)[:dm.NOPEN].tolist()
    dup[140] = dup[2]
    return {"low": list(range(dm.NOPEN)), "high": list(range(dm.NREST, dm.NPARTY)), "gap": list(range(257, 407)), "third": third,
            "random": rand, "dup": dup}


def _synthetic(k, rng, opened, big=False):
    """an image whose u16 are random below q (kept rows optionally with values in [q, 4095]), garbage in the rows to fill"""
    tab, total = dm.field_table(k)
    img = bytearray(rng.integers(0, dm.Q, size=total // 2, dtype=np.uint16).tobytes())
    img[tab[dm.F_I][0]:tab[dm.F_I][0] + 2 * dm.NOPEN] = np.array(opened, np.uint16).tobytes()
    if big:
        for f in dm.LISTED:
            off, size, cols = tab[f]
            v = np.frombuffer(bytes(img[off:off + dm.KEPT * cols * 2]), np.uint16).copy()
            sel = rng.random(len(v)) < 0.25
            v[sel] = rng.integers(dm.Q, 4096, size=int(sel.sum()), dtype=np.uint16)
            v[0], v[-1] = 4095, dm.Q
            img[off:off + dm.KEPT * cols * 2] = v.tobytes()
    return img


@pytest.mark.parametrize("k", KS)
def test_fill_device_against_the_model(k, torch):
    """n = 3, 2, 1 images (on a handle of max_batch 2, so n = 3 takes two launches) with the opened sets 0..149, 1304..1453, 257..406
    (nodes on both sides of a gap), every third party, a random set (kept values in [q, 4095] too) and one with a duplicate: status 1 and
    the image untouched.  Every byte outside the filled rows, and the guard bytes around every image, stay as they were."""
    api = _api()
    rng = np.random.default_rng(1900 + k)
    sets = _opened_sets(rng)
    ctx = api.Kosk(kyber_k=k, max_batch=2)
    total = dm.image_bytes(k)
    stride = (total + 15) // 16 * 16 + GUARD
    before = ctx.path_count(api.Kosk.PATH_DENSE_FILL)
    launches = 0
    for names, big in ((("low", "dup", "high"), False), (("gap", "third"), False), (("random",), True), (("dup",), False), (("random", "low", "third"), True)):
        n = len(names)
        imgs = [_synthetic(k, rng, sets[s], big) for s in names]
        buf = np.full(GUARD + n * stride, 0xA5, np.uint8)
        for b in range(n):
            buf[GUARD + b * stride:GUARD + b * stride + total] = np.frombuffer(bytes(imgs[b]), np.uint8)
        want = buf.copy()
        want_status = []
        for b in range(n):
            w = bytearray(imgs[b])
            want_status.append(dm.refill(k, w))
            want[GUARD + b * stride:GUARD + b * stride + total] = np.frombuffer(bytes(w), np.uint8)
        assert want_status == [1 if s == "dup" else 0 for s in names]
        d_buf = torch.from_numpy(buf).cuda()
        d_st = torch.full((n + 2,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert d_buf.data_ptr() % 16 == 0
        ctx.dense_fill_device(n, d_buf.data_ptr() + GUARD, stride, d_st.data_ptr() + 4)
        got = d_buf.cpu().numpy()
        st = d_st.cpu().numpy().tolist()
        assert st == [77] + want_status + [77], (k, names, st)
        assert got.tobytes() == want.tobytes(), (k, names, _first_diff(got.tobytes(), want.tobytes()))
        launches += (n + 1) // 2
    assert ctx.path_count(api.Kosk.PATH_DENSE_FILL) == before + launches
    with pytest.raises(api.KoskError):
        ctx.dense_fill_device(1, d_buf.data_ptr() + GUARD + 2, stride, d_st.data_ptr())   # images must be 16-byte aligned
    with pytest.raises(api.KoskError):
        ctx.dense_fill_device(1, d_buf.data_ptr() + GUARD, total - 16, d_st.data_ptr())
    ctx.close()


# ---- end to end
def _host_pack(api, k, pi):
    rc, rec = api.dense_pack(k, pi)
    assert rc == 0, rc
    return rec


@pytest.mark.parametrize("k", KS)
def test_keygen_dense_and_verify_dense(k, oracle, torch):
    api = _api()
    n = 3
    tapes = [oracle.tape_bytes_for(k, 190 + i) for i in range(n)]
    ctx = api.Kosk(kyber_k=k, max_batch=n)
    pks, sks, pis = ctx.verifiable_keygen(tapes)
    dpk, dsk, recs = ctx.verifiable_keygen_dense(tapes)
    assert (dpk, dsk) == (pks, sks)
    want = [_host_pack(api, k, pi) for pi in pis]
    for b in range(n):
        assert recs[b] == want[b], (k, b, _first_diff(recs[b], want[b]))
    before = ctx.path_count(api.Kosk.PATH_DENSE_FILL)
    assert ctx.verify_dense(recs, pks) == [True] * n
    assert ctx.path_count(api.Kosk.PATH_DENSE_FILL) == before + 1
    assert ctx.fetch_proofs(n) == pis, "the resident images after unpack + refill are not the original ones"
    # staged form, then the resident verifier; fetch packs what is resident
    ctx.stage_verifier_inputs_dense(recs[::-1], pks[::-1])
    assert ctx.verify_resident(n) == [True] * n
    assert ctx.fetch_proofs_dense(n) == recs[::-1]
    bad = bytearray(recs[1]); bad[100] ^= 0x10
    assert ctx.verify_dense([recs[0], bytes(bad), recs[2]], pks) == [True, False, True]
    # seeded form: the same bytes as the image call's proofs, packed
    seeds = [hashlib.sha3_256(b"kosk-dense-test-seed:%d" % b).digest() for b in range(n)]
    spk, ssk, spi = ctx.verifiable_keygen(seeds=seeds)
    tpk, tsk, srecs = ctx.verifiable_keygen_dense(seeds=seeds)
    assert (tpk, tsk) == (spk, ssk) and srecs == [_host_pack(api, k, pi) for pi in spi]
    assert ctx.verify_dense(srecs, spk) == [True] * n
    ctx.close()


def test_fetch_after_stage_prover_keys_with_a_rejected_key(oracle, torch):
    """the zero-witness proof left at a position with ok = 0 is a codeword too: the GPU pack (which does not check) equals the host
    codec (which does) at every position"""
    from tests import keyproof_cases as kc
    api = _api()
    k, n = 3, 4
    ctx = api.Kosk(kyber_k=k, max_batch=n)
    sks = [kc.honest(k, i)[1] for i in range(n)]
    sks[2] = kc.pk_swapped(k)
    tapes = [oracle.tape_bytes_for(k, 110 + i) for i in range(n)]
    assert ctx.stage_prover_keys(sks, tapes) == [True, True, False, True]
    ctx.prove_resident(n)
    pis = ctx.fetch_proofs(n)
    recs = ctx.fetch_proofs_dense(n)
    for b in range(n):
        assert api.dense_pack(k, pis[b]) == (0, recs[b]), b
    pks = [sk[384 * k:384 * k + ctx.pk_bytes] for sk in sks]
    assert ctx.verify_dense(recs, pks) == [True, True, False, True]
    ctx.close()


def test_armed_handle(oracle, torch):
    api = _api()
    k, n = 2, 3
    tapes = [oracle.tape_bytes_for(k, 120 + i) for i in range(n)]
    ctxs = [hashlib.sha3_256(b"kosk-dense-test-context:%d" % b).digest() for b in range(n)]
    ctx = api.Kosk(kyber_k=k, max_batch=n)
    ctx.set_contexts(ctxs)
    pks, sks, pis = ctx.verifiable_keygen(tapes)
    dpk, dsk, recs = ctx.verifiable_keygen_dense(tapes)
    assert (dpk, dsk) == (pks, sks) and recs == [_host_pack(api, k, pi) for pi in pis]
    assert ctx.verify_dense(recs, pks) == [True] * n
    ctx.set_contexts(ctxs[1:] + ctxs[:1])
    assert ctx.verify_dense(recs, pks) == [False] * n
    ctx.clear_contexts()
    assert ctx.verify_dense(recs, pks) == [False] * n
    ctx.set_contexts(ctxs[:2])
    with pytest.raises(api.KoskError):
        ctx.verify_dense(recs, pks)                     # armed with fewer contexts than proofs
    ctx.close()


@pytest.mark.parametrize("pinned", [False, True])
def test_chunked_calls_pinned_and_pageable(pinned, oracle, torch):
    """n = 5 through a handle of max_batch 2 (three chunks, the last ragged), records in pageable memory and in kosk_host_alloc memory"""
    api = _api()
    lib = api.lib
    k, n = 3, 5
    tapes = [oracle.tape_bytes_for(k, 170 + i) for i in range(n)]
    ref = api.Kosk(kyber_k=k, max_batch=n)
    pks, sks, pis = ref.verifiable_keygen(tapes)
    want = b"".join(_host_pack(api, k, pi) for pi in pis)
    cb = api.dense_proof_bytes(k)
    ctx = api.Kosk(kyber_k=k, max_batch=2)
    pk = C.create_string_buffer(ctx.pk_bytes * n); sk = C.create_string_buffer(ctx.sk_bytes * n); ok = C.create_string_buffer(n)
    if pinned:
        ptr = lib.kosk_host_alloc(cb * n)
        assert ptr
        out = C.c_void_p(ptr)
    else:
        buf = C.create_string_buffer(cb * n)
        out, ptr = buf, C.addressof(buf)
    pc0 = ctx.path_counts()
    assert lib.kosk_verifiable_keygen_batch_dense(ctx.handle, n, C.c_char_p(b"".join(tapes)), ctx.tape_bytes, pk, sk, out) == 0
    got = C.string_at(ptr, cb * n)
    assert pk.raw == b"".join(pks) and sk.raw == b"".join(sks)
    assert got == want, _first_diff(got, want)
    fills = ctx.path_count(api.Kosk.PATH_DENSE_FILL)
    assert lib.kosk_verify_batch_dense(ctx.handle, n, out, pk, ok) == 0 and ok.raw == b"\x01" * n
    assert ctx.path_count(api.Kosk.PATH_DENSE_FILL) == fills + 3
    pc1 = ctx.path_counts()
    assert pc1["copy_direct"] + pc1["copy_staged"] == pc0["copy_direct"] + pc0["copy_staged"] + 6   # one record copy per chunk and call
    if pinned:
        assert pc1["copy_direct"] == pc0["copy_direct"] + 6
    bad = bytearray(got); bad[4 * cb + 200] ^= 0x20
    C.memmove(ptr, bytes(bad), cb * n)
    assert lib.kosk_verify_batch_dense(ctx.handle, n, out, pk, ok) == 0 and ok.raw == b"\x01" * 4 + b"\x00"
    masks = ctx.fail_masks(n)
    st, img = api.dense_unpack(k, bytes(bad[4 * cb:5 * cb]))
    assert ref.verify(pis[:4] + [img], pks) == [True] * 4 + [False] and ref.fail_masks(n) == masks
    assert lib.kosk_verify_batch_dense(ctx.handle, 0, out, pk, ok) == 0
    if pinned:
        lib.kosk_host_free(C.c_void_p(ptr))
    ref.close(); ctx.close()


# ---- the contract: a dense record verifies exactly as the image it unpacks to
def _corruptions(k, rec, rng):
    """(what, record) with one byte changed (or one opened party replaced), about 40 of them"""
    lay, _ = dm.record_layout(k)
    out = []

    def flip(what, f, where):
        ro, rb = lay[f]
        r = bytearray(rec)
        r[ro + where % rb] ^= 1 << int(rng.integers(0, 8))
        out.append((what, bytes(r)))
    for f in dm.LISTED:                                  # kept rows of each listed field: first bytes, last bytes, somewhere
        rb = lay[f][1]
        for where in (0, rb - 2, int(rng.integers(0, rb))):
            flip("kept rows of field %d" % f, f, where)
    for i in range(3):
        flip("opened-party field 6", 6, int(rng.integers(0, lay[6][1])))
        flip("Tcomm", 4, int(rng.integers(0, lay[4][1])))
        flip("field 21", 21, int(rng.integers(0, lay[21][1])))
    for f in (0, 22, 23):
        for i in range(2):
            flip("field %d" % f, f, int(rng.integers(0, lay[f][1])))
    ro, rb = lay[dm.F_I]
    opened = dm.unpack12(rec[ro:ro + rb], dm.NOPEN)
    free = sorted(set(range(dm.NPARTY)) - set(opened.tolist()))
    for what, pos, val in (("I: another unopened party", 0, free[0]), ("I: another unopened party", 149, free[-1]), ("I: another unopened party", 70, free[600]),
                           ("I: duplicate", 9, int(opened[100])), ("I: out of range", 33, dm.NPARTY)):
        o2 = opened.copy(); o2[pos] = val
        r = bytearray(rec); r[ro:ro + rb] = dm.pack12(o2).tobytes()
        out.append((what, bytes(r)))
    return out


@pytest.mark.parametrize("k", [3, 2])
def test_dense_records_verify_as_their_images(k, oracle, torch):
    api = _api()
    rng = np.random.default_rng(1950 + k)
    tape = oracle.tape_bytes_for(k, 0)
    pk, sk, pi = oracle.verifiable_keygen(k, tape)[:3]
    rec = _host_pack(api, k, pi)
    cases = [("intact", rec)] + _corruptions(k, rec, rng)
    n = len(cases)
    assert 38 <= n <= 48
    recs = [c[1] for c in cases]
    unpacked = [api.dense_unpack(k, r) for r in recs]
    assert [u[0] for u in unpacked] == [1 if c[0] in ("I: duplicate", "I: out of range") else 0 for c in cases]
    imgs = [u[1] for u in unpacked]
    assert imgs[0] == pi
    pks = [pk] * n
    for strict in (0, 1):
        ctx = api.Kosk(kyber_k=k, max_batch=n, strict_encoding=strict)
        want = ctx.verify(imgs, pks)
        want_masks = ctx.fail_masks(n)
        got = ctx.verify_dense(recs, pks)
        got_masks = ctx.fail_masks(n)
        for b in range(n):
            assert (got[b], got_masks[b]) == (want[b], want_masks[b]), (k, strict, b, cases[b][0], hex(got_masks[b]), hex(want_masks[b]))
        assert want[0] and not want_masks[0] and not all(want)
        ctx.close()
