"""GPU tests of the dense wire format kosk-dense-v2 (csrc/kosk_dense.hip: k_dense2_setup, k_dense2_fill, k_dense2_check;
the v2 field plan of the pack / unpack kernels and the fourth format of the transcoder in csrc/kosk_compact.hip; the five _fmt calls).
References: the numpy model tests/dense2_model.py for the refill and the check, the host codecs (pinned to that model by
tests/test_dense2_host.py) for whole records, the image calls for verify bits and fail masks.  Every comparison is exact.
Handles of max_batch 2 and calls of n = 5, so that three chunks or sub-batches run."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests import dense2_cases as dc
from tests import dense2_model as d2
from tests import dense_model as dm

pytestmark = pytest.mark.gpu

KS = (2, 3, 4)
GUARD = 256
FMT2 = dc.FMT_DENSE2
FIVE = ("first150", "dup", "last150", "gap", "third")


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
    if len(a) != len(b):
        return ("length", len(a), len(b))
    d = np.nonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8))[0]
    return None if len(d) == 0 else (int(d[0]), len(d))


def _device_images(torch, imgs, total, stride):
    n = len(imgs)
    buf = np.full(GUARD + n * stride, 0xA5, np.uint8)
    for b in range(n):
        buf[GUARD + b * stride:GUARD + b * stride + total] = np.frombuffer(bytes(imgs[b]), np.uint8)
    d_buf = torch.from_numpy(buf).cuda()
    d_st = torch.full((n + 2,), 77, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    assert d_buf.data_ptr() % 16 == 0
    return buf, d_buf, d_st


# ---- 1. the refill
@pytest.mark.parametrize("k", KS)
def test_fill_device_against_the_model(k, torch):
    """synthetic images (random kept rows, in two of them a quarter of the kept values in [q, 4095] and 4095 at both ends) on the opened
    sets 0..149, 1304..1453, 257..406, every third party, a random one and one with a duplicated entry (status 1, image untouched); the
    stride above the image size, guard bytes around every image: every byte outside the refilled rows is unchanged"""
    api = _api()
    rng = np.random.default_rng(3000 + k)
    sets = dc.opened_lists(rng)
    ctx = api.Kosk(kyber_k=k, max_batch=2)
    total = d2.image_bytes(k)
    stride = (total + 15) // 16 * 16 + GUARD
    fills, v1 = ctx.path_count(api.Kosk.PATH_DENSE2_FILL), ctx.path_count(api.Kosk.PATH_DENSE_FILL)
    launches = 0
    for names, big in ((FIVE, False), (("random", "third"), True)):
        n = len(names)
        imgs = [dc.synthetic(k, rng, sets[s], big) for s in names]
        buf, d_buf, d_st = _device_images(torch, imgs, total, stride)
        want = buf.copy()
        want_status = []
        for b in range(n):
            w = bytearray(imgs[b])
            want_status.append(d2.refill(k, w))
            want[GUARD + b * stride:GUARD + b * stride + total] = np.frombuffer(bytes(w), np.uint8)
        assert want_status == [1 if s == "dup" else 0 for s in names]
        ctx.dense2_fill_device(n, d_buf.data_ptr() + GUARD, stride, d_st.data_ptr() + 4)
        got = d_buf.cpu().numpy()
        st = d_st.cpu().numpy().tolist()
        assert st == [77] + want_status + [77], (k, names, st)
        assert got.tobytes() == want.tobytes(), (k, names, _first_diff(got.tobytes(), want.tobytes()))
        launches += (n + 1) // 2
    assert ctx.path_count(api.Kosk.PATH_DENSE2_FILL) == fills + launches and ctx.path_count(api.Kosk.PATH_DENSE_FILL) == v1
    with pytest.raises(api.KoskError):
        ctx.dense2_fill_device(1, d_buf.data_ptr() + GUARD + 2, stride, d_st.data_ptr())   # images must be 16-byte aligned
    with pytest.raises(api.KoskError):
        ctx.dense2_fill_device(1, d_buf.data_ptr() + GUARD, total - 16, d_st.data_ptr())
    ctx.close()


# ---- 2. the codeword check
@pytest.mark.parametrize("k", KS)
def test_check_device_against_the_model(k, torch):
    """status 0 on codewords (1 for the duplicate in I), 2 for single-u16 changes (tests/dense2_cases.check_mutations), the neighbours of
    every field as the model says; four changed images per call of n = 5.  The images and the status words around the n written ones are
    unchanged after every call."""
    api = _api()
    rng = np.random.default_rng(3010 + k)
    sets = dc.opened_lists(rng)
    total = d2.image_bytes(k)
    stride = (total + 15) // 16 * 16 + GUARD
    base = []
    for name in FIVE:
        img = dc.synthetic(k, rng, sets[name], big=name == "gap")
        if name != "dup":
            assert d2.refill(k, img) == 0
        base.append(bytes(img))
    clean = [1 if s == "dup" else 0 for s in FIVE]
    ctx = api.Kosk(kyber_k=k, max_batch=2)
    checks = ctx.path_count(api.Kosk.PATH_DENSE2_CHECK)
    calls = 0

    def run(imgs):
        nonlocal calls
        buf, d_buf, d_st = _device_images(torch, imgs, total, stride)
        ctx.dense2_check_device(len(imgs), d_buf.data_ptr() + GUARD, stride, d_st.data_ptr() + 4)
        calls += 1
        st = d_st.cpu().numpy().tolist()
        assert st[0] == 77 and st[-1] == 77, st
        got = d_buf.cpu().numpy()
        assert got.tobytes() == buf.tobytes(), ("the check wrote to the images", k, _first_diff(got.tobytes(), buf.tobytes()))
        return st[1:-1]

    assert run(base) == clean == [dc.model_check(k, b) for b in base]
    slots = [b for b in range(5) if FIVE[b] != "dup"]
    muts = [dc.check_mutations(k, base[b]) for b in range(5)]
    count = len(muts[0])
    assert count == 18 + 2 + 2 + 18
    for i0 in range(0, count, 4):
        imgs, want, what = list(base), list(clean), []
        for j, i in enumerate(range(i0, min(i0 + 4, count))):
            b = slots[(j + i0 // 4) % 4]                     # every case meets another chunk position than its neighbours
            name, off, val, stated = muts[b][i]
            img = bytearray(base[b])
            dc.put16(img, off, val)
            want[b] = dc.model_check(k, img)
            assert stated is None or stated == want[b], (k, name, stated, want[b])
            imgs[b] = bytes(img)
            what.append((b, name))
        st = run(imgs)
        assert st == want, (k, what, st, want)
    assert ctx.path_count(api.Kosk.PATH_DENSE2_CHECK) == checks + 3 * calls
    assert ctx.path_count(api.Kosk.PATH_DENSE_CHECK) == 0 and ctx.path_count(api.Kosk.PATH_DENSE2_FILL) == 0
    ctx.close()


# ---- 3. end to end through the five _fmt calls
def _host_pack(api, k, pi):
    rc, rec = api.proof_dense2_pack(k, pi)
    assert rc == 0, rc
    return rec


@pytest.mark.parametrize("k,pinned", [(2, False), (3, True), (4, False), (3, False)])
def test_fmt_calls_end_to_end(k, pinned, oracle, torch):
    api = _api()
    lib = api.lib
    n = 5
    tapes = [oracle.tape_bytes_for(k, 300 + i) for i in range(n)]
    seeds = [hashlib.sha3_256(b"kosk-dense2-test-seed:%d" % b).digest() for b in range(n)]
    ref = api.Kosk(kyber_k=k, max_batch=n)
    pks, sks, pis = ref.verifiable_keygen(tapes)
    want = b"".join(_host_pack(api, k, pi) for pi in pis)
    spk, ssk, spi = ref.verifiable_keygen(seeds=seeds)
    swant = b"".join(_host_pack(api, k, pi) for pi in spi)
    rb = api.format_bytes(k, FMT2)
    ctx = api.Kosk(kyber_k=k, max_batch=2)
    h = ctx.handle
    pk = C.create_string_buffer(ctx.pk_bytes * n); sk = C.create_string_buffer(ctx.sk_bytes * n); ok = C.create_string_buffer(n)
    if pinned:
        ptr = lib.kosk_host_alloc(rb * n)
        assert ptr
        out = C.c_void_p(ptr)
    else:
        buf = C.create_string_buffer(rb * n)
        out, ptr = buf, C.addressof(buf)
    pc0 = ctx.path_counts()
    assert lib.kosk_verifiable_keygen_batch_fmt(h, FMT2, n, C.c_char_p(b"".join(tapes)), ctx.tape_bytes, pk, sk, out) == 0, lib.kosk_last_error(h)
    got = C.string_at(ptr, rb * n)
    assert pk.raw == b"".join(pks) and sk.raw == b"".join(sks)
    assert got == want, _first_diff(got, want)
    fills = ctx.path_count(api.Kosk.PATH_DENSE2_FILL)
    assert lib.kosk_verify_batch_fmt(h, FMT2, n, out, pk, ok) == 0 and ok.raw == b"\x01" * n
    assert ctx.fail_masks(n) == [0] * n
    assert ctx.path_count(api.Kosk.PATH_DENSE2_FILL) == fills + 3 and ctx.path_count(api.Kosk.PATH_DENSE_FILL) == 0
    pc1 = ctx.path_counts()
    assert pc1["copy_direct"] + pc1["copy_staged"] == pc0["copy_direct"] + pc0["copy_staged"] + 6   # one record copy per chunk and call
    if pinned:
        assert pc1["copy_direct"] == pc0["copy_direct"] + 6
    # seeded
    assert lib.kosk_verifiable_keygen_seeded_batch_fmt(h, FMT2, n, C.c_char_p(b"".join(seeds)), 32, pk, sk, out) == 0
    got = C.string_at(ptr, rb * n)
    assert pk.raw == b"".join(spk) and sk.raw == b"".join(ssk) and got == swant, _first_diff(got, swant)
    assert lib.kosk_verify_batch_fmt(h, FMT2, n, out, pk, ok) == 0 and ok.raw == b"\x01" * n
    assert lib.kosk_verify_batch_fmt(h, FMT2, 0, out, pk, ok) == 0
    # staging and fetching resident proofs: n <= max_batch
    recs = [want[b * rb:(b + 1) * rb] for b in range(n)]
    assert lib.kosk_stage_verifier_inputs_fmt(h, FMT2, 2, recs[3] + recs[1], pks[3] + pks[1]) == 0
    assert ctx.verify_resident(2) == [True, True]
    assert ctx.fetch_proofs(2) == [pis[3], pis[1]], "the resident images after unpack + refill are not the original ones"
    two = C.create_string_buffer(2 * rb)
    assert lib.kosk_fetch_proofs_fmt(h, FMT2, 2, two) == 0 and two.raw == recs[3] + recs[1]
    # a resident key generation, then fetch
    assert ctx.verifiable_keygen_resident(tapes[:2]) == 2
    assert ctx.keys(2) == (pks[:2], sks[:2])
    assert ctx.fetch_proofs_dense2(2) == recs[:2]
    # the binding's methods run the same calls
    assert ctx.verify_dense2(recs, pks) == [True] * n
    bad = bytearray(recs[4]); bad[200] ^= 0x20
    assert ctx.verify_dense2(recs[:4] + [bytes(bad)], pks) == [True] * 4 + [False]
    masks = ctx.fail_masks(n)
    st, img = api.proof_dense2_unpack(k, bytes(bad))
    assert ref.verify(pis[:4] + [img], pks) == [True] * 4 + [False] and ref.fail_masks(n) == masks
    if pinned:
        lib.kosk_host_free(C.c_void_p(ptr))
    ref.close(); ctx.close()


def test_armed_handle(oracle, torch):
    api = _api()
    k, n = 2, 5
    tapes = [oracle.tape_bytes_for(k, 320 + i) for i in range(n)]
    ctxs = [hashlib.sha3_256(b"kosk-dense2-test-context:%d" % b).digest() for b in range(n)]
    ctx = api.Kosk(kyber_k=k, max_batch=2)
    ctx.set_contexts(ctxs)
    pks, sks, pis = ctx.verifiable_keygen(tapes)
    dpk, dsk, recs = ctx.verifiable_keygen_dense2(tapes)
    assert (dpk, dsk) == (pks, sks) and recs == [_host_pack(api, k, pi) for pi in pis]
    assert ctx.verify_dense2(recs, pks) == [True] * n
    ctx.set_contexts(ctxs[1:] + ctxs[:1])
    assert ctx.verify_dense2(recs, pks) == [False] * n
    ctx.clear_contexts()
    assert ctx.verify_dense2(recs, pks) == [False] * n
    ctx.set_contexts(ctxs[:2])
    with pytest.raises(api.KoskError):
        ctx.verify_dense2(recs, pks)                     # armed with fewer contexts than proofs
    ctx.close()


def test_zero_witness_proof_of_a_rejected_key_packs(oracle, torch):
    """the zero-witness proof left at a position with ok = 0 is a codeword of v2 too: the GPU pack (which does not check) equals the host
    codec (which does, status 0) at every position"""
    from tests import keyproof_cases as kc
    api = _api()
    k, n = 3, 4
    ctx = api.Kosk(kyber_k=k, max_batch=n)
    sks = [kc.honest(k, i)[1] for i in range(n)]
    sks[2] = kc.pk_swapped(k)
    tapes = [oracle.tape_bytes_for(k, 330 + i) for i in range(n)]
    assert ctx.stage_prover_keys(sks, tapes) == [True, True, False, True]
    ctx.prove_resident(n)
    pis = ctx.fetch_proofs(n)
    recs = ctx.fetch_proofs_dense2(n)
    for b in range(n):
        assert api.proof_dense2_pack(k, pis[b]) == (0, recs[b]), b
    pks = [sk[384 * k:384 * k + ctx.pk_bytes] for sk in sks]
    assert ctx.verify_dense2(recs, pks) == [True, True, False, True]
    ctx.close()


# ---- 4. a v2 record verifies exactly as the image it unpacks to
def _corruptions(k, rec, rng):
    """(what, record): kept rows of each of the four fields (first and last bytes), the opened list, the two digest fields, and a value >= q
    in a kept row"""
    lay, _ = d2.record_layout(k)
    out = []

    def flip(what, f, where):
        ro, rb = lay[f]
        r = bytearray(rec)
        r[ro + where % rb] ^= 1 << int(rng.integers(0, 8))
        out.append((what, bytes(r)))
    for f in (15, 16, 21, 22):
        flip("first kept bytes of field %d" % f, f, 0)
        flip("last kept value of field %d" % f, f, lay[f][1] - 3)      # the low byte of the last pair's first value: never padding
    flip("Tcomm", 4, int(rng.integers(0, lay[4][1])))
    flip("comm", 23, int(rng.integers(0, lay[23][1])))
    ro, rb = lay[d2.F_I]
    opened = d2.unpack12(rec[ro:ro + rb], d2.NOPEN)
    free = sorted(set(range(d2.NPARTY)) - set(opened.tolist()))
    for what, pos, val in (("I: another unopened party", 70, free[600]), ("I: duplicate", 9, int(opened[100])), ("I: out of range", 33, d2.NPARTY)):
        o2 = opened.copy(); o2[pos] = val
        r = bytearray(rec); r[ro:ro + rb] = d2.pack12(o2).tobytes()
        out.append((what, bytes(r)))
    ro, rb = lay[21]
    nv = d2.stored_values(k)[21]
    vals = d2.unpack12(rec[ro:ro + rb], nv).copy()
    i = next(i for i in range(100, nv) if vals[i] + d2.Q < 4096)
    vals[i] += d2.Q
    r = bytearray(rec); r[ro:ro + rb] = d2.pack12(vals).tobytes()
    out.append(("a value >= q in a kept row of field 21", bytes(r)))
    return out


@pytest.mark.parametrize("k", KS)
def test_corrupted_records_verify_as_their_images(k, oracle, torch):
    api = _api()
    rng = np.random.default_rng(3050 + k)
    tape = oracle.tape_bytes_for(k, 0)
    pk, sk, pi = oracle.verifiable_keygen(k, tape)[:3]
    rec = _host_pack(api, k, pi)
    cases = [("intact", rec)] + _corruptions(k, rec, rng)
    n = len(cases)
    assert n == 15
    recs = [c[1] for c in cases]
    unpacked = [api.proof_dense2_unpack(k, r) for r in recs]
    assert [u[0] for u in unpacked] == [1 if c[0] in ("I: duplicate", "I: out of range") else 0 for c in cases]
    imgs = [u[1] for u in unpacked]
    assert imgs[0] == pi
    pks = [pk] * n
    for strict in (0, 1):
        ref = api.Kosk(kyber_k=k, max_batch=n, strict_encoding=strict)
        want = ref.verify(imgs, pks)
        want_masks = ref.fail_masks(n)
        ref.close()
        ctx = api.Kosk(kyber_k=k, max_batch=2, strict_encoding=strict)
        got = ctx.verify_dense2(recs, pks)
        got_masks = ctx.fail_masks(n)
        ctx.close()
        for b in range(n):
            assert (got[b], got_masks[b]) == (want[b], want_masks[b]), (k, strict, b, cases[b][0], hex(got_masks[b]), hex(want_masks[b]))
        assert want[0] and not want_masks[0] and not all(want)


# ---- 5. the fourth format of kosk_transcode_batch
def _batches(api, k):
    """{(from, to): [names or records]} for the six pairs that involve format 4: calls of n = 5"""
    cases = dc.transcode_images(k)
    img = lambda name: cases[name][0]
    host = lambda frm, to, rec: dc.host_transcode(api, k, frm, to, rec)
    out = {}
    out[0, 4] = [[img(s) for s in ("ok", "kept_big", "eta_row300_big", "bad_I", "u_row1000_changed")],
                 [img(s) for s in ("eta_other_secret", "t_row1000_changed", "u_row900_big", "ok", "kept_big")]]
    out[1, 4] = [[host(0, 1, img(s))[1] for s in ("ok", "u_row1000_changed", "bad_I", "eta_other_secret", "t_row1000_changed")]]
    v1 = host(0, 2, img("ok"))[1]
    out[2, 4] = [[v1, host(0, 2, img("u_row1000_changed"))[1], host(0, 2, img("eta_other_secret"))[1],
                  dc.bad_I_record(k, v1, dm.record_layout(k)[0], "dup"), v1]]
    v2 = host(0, 4, img("ok"))[1]
    lay2 = d2.record_layout(k)[0]
    from4 = [v2, dc.bad_I_record(k, v2, lay2, "dup"), v2, dc.bad_I_record(k, v2, lay2, "range"), v2]
    for to in (0, 1, 2):
        out[4, to] = [from4]
    return out


@pytest.mark.parametrize("k", KS)
def test_transcode_pairs_with_format_4(k, torch):
    api = _api()
    ctx = api.Kosk(kyber_k=k, max_batch=2)
    c2, c1 = ctx.path_count(api.Kosk.PATH_DENSE2_CHECK), ctx.path_count(api.Kosk.PATH_DENSE_CHECK)
    f2, f1 = ctx.path_count(api.Kosk.PATH_DENSE2_FILL), ctx.path_count(api.Kosk.PATH_DENSE_FILL)
    seen = set()
    for (frm, to), calls in _batches(api, k).items():
        for batch in calls:
            want = [dc.host_transcode(api, k, frm, to, rec) for rec in batch]
            st, out = ctx.transcode(batch, frm, to)
            where = (k, dc.FMT_NAMES[frm], dc.FMT_NAMES[to])
            assert st == [w[0] for w in want], (where, st, [w[0] for w in want])
            for b in range(5):
                assert len(out[b]) == api.format_bytes(k, to)
                if st[b] < 0:
                    assert out[b] == bytes(len(out[b])), (where, b, "a refused record is not all zero")
                else:
                    assert out[b] == want[b][1], (where, b, _first_diff(out[b], want[b][1]))
                seen.add((frm, to, st[b]))
            c2 += 3 if to == 4 else 0
            c1 += 3 if to == 2 else 0
            f2 += 3 if frm == 4 else 0
            f1 += 3 if frm == 2 else 0
    for want in ((0, 4, 0), (0, 4, -1), (0, 4, -2), (1, 4, 0), (1, 4, -2), (2, 4, 0), (2, 4, -2), (4, 0, 0), (4, 0, 1), (4, 1, 1), (4, 2, 0), (4, 2, -2)):
        assert want in seen, want
    assert (ctx.path_count(api.Kosk.PATH_DENSE2_CHECK), ctx.path_count(api.Kosk.PATH_DENSE_CHECK)) == (c2, c1)
    assert (ctx.path_count(api.Kosk.PATH_DENSE2_FILL), ctx.path_count(api.Kosk.PATH_DENSE_FILL)) == (f2, f1)
    # dense -> dense2 -> dense, byte for byte
    pi = dc.oracle_proof(k)
    v1 = [dc.host_transcode(api, k, 0, 2, pi)[1]] * 3
    st, v2 = ctx.transcode(v1, 2, 4)
    assert st == [0, 0, 0] and v2 == [_host_pack(api, k, pi)] * 3
    assert ctx.transcode(v2, 4, 2) == ([0, 0, 0], v1)
    # 3 and 5 are no formats; 4 to 4 is refused like every from == to
    src = C.create_string_buffer(pi, len(pi)); dst = C.create_string_buffer(len(pi)); stw = (C.c_int32 * 1)(55)
    for frm, to, text in ((3, 4, b"format"), (4, 3, b"format"), (5, 0, b"format"), (0, 5, b"format"), (4, 4, b"same format")):
        assert api.lib.kosk_transcode_batch(ctx.handle, 1, frm, src, to, dst, stw) == -1
        assert text in api.lib.kosk_last_error(ctx.handle), (frm, to)
    assert stw[0] == 55
    ctx.close()


def test_transcoding_leaves_the_resident_state(oracle, torch):
    api = _api()
    k, n = 3, 2
    tapes = [oracle.tape_bytes_for(k, 340 + i) for i in range(n)]
    coins = [hashlib.sha3_256(b"kosk-dense2-test-coins:%d" % b).digest() for b in range(n)]
    ctx = api.Kosk(kyber_k=k, max_batch=n)
    pks, sks, pis = ctx.verifiable_keygen(tapes)
    assert ctx.verify_resident_pk(n) == [True] * n

    def snapshot():
        return (ctx.fetch_proofs(n), ctx.fetch_proofs_dense2(n), ctx.verify_resident_pk(n), ctx.fail_masks(n), ctx.kem_enc_verified(n, coins))
    first = snapshot()
    assert first[0] == pis and first[4][2] == [True] * n
    for (frm, to), calls in _batches(api, k).items():
        batch = calls[0][:3]
        st, out = ctx.transcode(batch, frm, to)
        assert st == [dc.host_transcode(api, k, frm, to, rec)[0] for rec in batch]
        assert ctx.kem_enc_verified(n, coins) == first[4], (frm, to)
        assert snapshot() == first, (frm, to)
    st, recs = ctx.transcode(pis, api.FMT_IMAGE, api.FMT_DENSE2)
    assert st == [0] * n and recs == first[1]
    ctx.close()


# ---- 6. counters and the old formats
def test_fmt_calls_with_the_old_formats_are_the_named_calls(oracle, torch):
    api = _api()
    lib = api.lib
    k, n = 3, 5
    tapes = b"".join(oracle.tape_bytes_for(k, 350 + i) for i in range(n))
    seeds = b"".join(hashlib.sha3_256(b"kosk-dense2-test-old:%d" % b).digest() for b in range(n))
    ctx = api.Kosk(kyber_k=k, max_batch=2)
    h = ctx.handle
    pk = C.create_string_buffer(ctx.pk_bytes * n); sk = C.create_string_buffer(ctx.sk_bytes * n)
    ok_a = C.create_string_buffer(n); ok_b = C.create_string_buffer(n)
    for fmt, sfx, fill_id in ((api.FMT_COMPACT, "compact", None), (api.FMT_DENSE, "dense", api.Kosk.PATH_DENSE_FILL)):
        rb = api.format_bytes(k, fmt)
        a = C.create_string_buffer(rb * n); b = C.create_string_buffer(rb * n)
        named = {name: getattr(lib, "kosk_" + name + "_" + sfx) for name in ("verifiable_keygen_batch", "verifiable_keygen_seeded_batch", "verify_batch",
                                                                             "fetch_proofs", "stage_verifier_inputs")}
        assert named["verifiable_keygen_batch"](h, n, tapes, ctx.tape_bytes, pk, sk, a) == 0
        assert lib.kosk_verifiable_keygen_batch_fmt(h, fmt, n, tapes, ctx.tape_bytes, pk, sk, b) == 0 and a.raw == b.raw
        assert named["verifiable_keygen_seeded_batch"](h, n, seeds, 32, pk, sk, a) == 0
        assert lib.kosk_verifiable_keygen_seeded_batch_fmt(h, fmt, n, seeds, 32, pk, sk, b) == 0 and a.raw == b.raw
        assert named["verifiable_keygen_seeded_batch"](h, n, seeds, 31, pk, sk, a) == -1
        text = lib.kosk_last_error(h).split(b": ", 1)[1]
        assert lib.kosk_verifiable_keygen_seeded_batch_fmt(h, fmt, n, seeds, 31, pk, sk, b) == -1 and lib.kosk_last_error(h).split(b": ", 1)[1] == text
        before = [ctx.path_count(i) for i in (14, 22, 23, 24)]
        assert named["verify_batch"](h, n, a, pk, ok_a) == 0 and lib.kosk_verify_batch_fmt(h, fmt, n, a, pk, ok_b) == 0
        assert ok_a.raw == ok_b.raw == b"\x01" * n
        after = [ctx.path_count(i) for i in (14, 22, 23, 24)]
        assert after == [before[0] + (6 if fill_id == 14 else 0), before[1], before[2], before[3]]
        assert named["verify_batch"](h, n, a, None, ok_a) == -1 and lib.kosk_verify_batch_fmt(h, fmt, n, a, None, ok_b) == -1
        assert named["stage_verifier_inputs"](h, 2, a, pk) == 0 and named["fetch_proofs"](h, 2, b) == 0
        one = b.raw[:2 * rb]
        assert lib.kosk_stage_verifier_inputs_fmt(h, fmt, 2, a, pk) == 0 and lib.kosk_fetch_proofs_fmt(h, fmt, 2, b) == 0
        assert b.raw[:2 * rb] == one == a.raw[:2 * rb]
        assert named["fetch_proofs"](h, 3, b) == -1 and lib.kosk_fetch_proofs_fmt(h, fmt, 3, b) == -1      # n above max_batch
        assert named["stage_verifier_inputs"](h, 3, a, pk) == -1 and lib.kosk_stage_verifier_inputs_fmt(h, fmt, 3, a, pk) == -1
    # any other fmt is refused, with a text that says why
    a = C.create_string_buffer(api.proof_bytes(k) * n)
    for fmt in (0, 3, 5, -1):
        for rc in (lib.kosk_verifiable_keygen_batch_fmt(h, fmt, n, tapes, ctx.tape_bytes, pk, sk, a),
                   lib.kosk_verifiable_keygen_seeded_batch_fmt(h, fmt, n, seeds, 32, pk, sk, a),
                   lib.kosk_verify_batch_fmt(h, fmt, n, a, pk, ok_a), lib.kosk_fetch_proofs_fmt(h, fmt, 2, a),
                   lib.kosk_stage_verifier_inputs_fmt(h, fmt, 2, a, pk)):
            assert rc == -1 and b"format" in lib.kosk_last_error(h), fmt
    ctx.close()


def test_counters_and_kem_enc_verified_after_v2_staging(oracle, torch):
    """ids 23 / 24 move by one per staged chunk or sub-batch of v2 work and 14 / 22 stay; kosk_kem_enc_verified is refused once a v2 verifier
    staging call has replaced the resident keys"""
    api = _api()
    k, n = 2, 5
    tapes = [oracle.tape_bytes_for(k, 360 + i) for i in range(n)]
    coins = [hashlib.sha3_256(b"kosk-dense2-test-kem:%d" % b).digest() for b in range(2)]
    ctx = api.Kosk(kyber_k=k, max_batch=2)
    ids = (14, 22, 23, 24)
    pks, sks, recs = ctx.verifiable_keygen_dense2(tapes)
    assert [ctx.path_count(i) for i in ids] == [0, 0, 0, 0]          # packing refills nothing
    assert ctx.verify_dense2(recs, pks) == [True] * n
    assert [ctx.path_count(i) for i in ids] == [0, 0, 3, 0]
    ctx.stage_verifier_inputs_dense2(recs[:2], pks[:2])
    assert [ctx.path_count(i) for i in ids] == [0, 0, 4, 0]
    st, imgs = ctx.transcode(recs, FMT2, api.FMT_IMAGE)
    assert st == [0] * n and [ctx.path_count(i) for i in ids] == [0, 0, 7, 0]
    st, back = ctx.transcode(imgs, api.FMT_IMAGE, FMT2)
    assert (st, back) == ([0] * n, recs) and [ctx.path_count(i) for i in ids] == [0, 0, 7, 3]
    assert ctx.verify_dense2(recs[:2], pks[:2]) == [True, True]
    assert ctx.kem_enc_verified(2, coins)[2] == [True, True]
    ctx.stage_verifier_inputs_dense2(recs[2:4], pks[2:4])
    with pytest.raises(api.KoskError):
        ctx.kem_enc_verified(2, coins)
    ctx.close()
