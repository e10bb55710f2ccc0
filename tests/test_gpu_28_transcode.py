"""GPU tests of the transcoder between the wire formats (kosk_transcode_batch, kosk_dense_check_device; k_dense_check in
csrc/kosk_dense.hip and the host plumbing in csrc/kosk_compact.hip).  References: the host codecs for whole records (held to the numpy model by
tests/test_transcode_host.py) and tests/dense_model.py for the check.  Every comparison is exact; every case is a defined return code."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests import dense_model as dm
from tests import transcode_cases as tc

pytestmark = pytest.mark.gpu

KS = tc.KS
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
    if len(a) != len(b):
        return ("length", len(a), len(b))
    d = np.nonzero(np.frombuffer(a, np.uint8) != np.frombuffer(b, np.uint8))[0]
    return None if len(d) == 0 else (int(d[0]), len(d))


# ---- 1. kernel level: kosk_dense_check_device against the model
@pytest.mark.parametrize("k", KS)
def test_check_device_against_the_model(k, torch):
    """n = 3, 2, 1 images on a handle of max_batch 2 (n = 3 takes two launches), the six opened sets of test_gpu_19_dense.py, images made
    representable by dense_model.refill (kept values in [q, 4095] in one of them).  Clean images give 0 (1 for the duplicate in I); then one
    image of a batch gets one changed u16 per case (tests/transcode_cases.check_mutations) and the status is the model's: 2 for every filled
    row and for a changed kept value, 0 for the u16 of a neighbouring field that shares a 16-byte chunk with filled rows.  The status words
    around the n written ones and every byte of the image buffer, guard bytes included, are unchanged after every call."""
    api = _api()
    rng = np.random.default_rng(2810 + k)
    sets = tc.opened_sets(rng)
    total = dm.image_bytes(k)
    stride = (total + 15) // 16 * 16 + GUARD
    base = {}
    for name in ("low", "high", "gap", "third", "random"):
        img = tc.synthetic(k, rng, sets[name], big=name == "random")
        assert dm.refill(k, img) == 0
        base[name] = bytes(img)
    base["dup"] = bytes(tc.synthetic(k, rng, sets["dup"]))
    groups = (("low", "dup", "high"), ("gap", "third"), ("random",), ("dup",))
    ctx = api.Kosk(kyber_k=k, max_batch=2)
    before = ctx.path_count(api.Kosk.PATH_DENSE_CHECK)
    launches = 0

    def run(names, imgs):
        nonlocal launches
        n = len(names)
        buf = np.full(GUARD + n * stride, 0xA5, np.uint8)
        for b in range(n):
            buf[GUARD + b * stride:GUARD + b * stride + total] = np.frombuffer(imgs[b], np.uint8)
        d_buf = torch.from_numpy(buf).cuda()
        d_st = torch.full((n + 2,), 77, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        assert d_buf.data_ptr() % 16 == 0
        ctx.dense_check_device(n, d_buf.data_ptr() + GUARD, stride, d_st.data_ptr() + 4)
        launches += (n + 1) // 2
        st = d_st.cpu().numpy().tolist()
        assert st[0] == 77 and st[-1] == 77, (k, names, st)
        got = d_buf.cpu().numpy()
        assert got.tobytes() == buf.tobytes(), ("the check wrote to the images", k, names, _first_diff(got.tobytes(), buf.tobytes()))
        return st[1:-1], d_buf, d_st

    for names in groups:
        st, d_buf, d_st = run(names, [base[s] for s in names])
        assert st == [1 if s == "dup" else 0 for s in names], (k, names, st)
        assert st == [tc.model_check(k, base[s]) for s in names]
    # one changed u16 per case, the target walking over every position of the n = 3, 2, 1 batches
    targets = [(0, 0), (1, 1), (2, 0), (0, 2), (1, 0)]
    muts = None
    for i in range(32):
        g, pos = targets[i % len(targets)]
        names = groups[g]
        img0 = base[names[pos]]
        muts = tc.check_mutations(k, img0)
        if i >= len(muts):
            break
        what, off, val, stated = muts[i]
        img = bytearray(img0)
        tc.put16(img, off, val)
        want = tc.model_check(k, img)
        assert stated == want, (k, what, stated, want)
        imgs = [base[s] for s in names]
        imgs[pos] = bytes(img)
        st, d_buf, d_st = run(names, imgs)
        assert st == [want if b == pos else (1 if s == "dup" else 0) for b, s in enumerate(names)], (k, what, names, pos, st)
    assert len(muts) == 31 and i == 31
    assert ctx.path_count(api.Kosk.PATH_DENSE_CHECK) == before + launches
    assert ctx.path_count(api.Kosk.PATH_DENSE_FILL) == 0
    with pytest.raises(api.KoskError):
        ctx.dense_check_device(1, d_buf.data_ptr() + GUARD + 2, stride, d_st.data_ptr())   # images must be 16-byte aligned
    with pytest.raises(api.KoskError):
        ctx.dense_check_device(1, d_buf.data_ptr() + GUARD, total - 16, d_st.data_ptr())   # a stride below one image
    ctx.close()


# ---- 2. kosk_transcode_batch against the host codecs, all six pairs
@pytest.mark.parametrize("k", KS)
def test_all_pairs_against_the_host_codecs(k, torch):
    """calls of n = 5 on a handle of max_batch 2 (three chunks): statuses and, for status >= 0, bytes are the host codecs' composition; a
    record with a negative status is all zero.  Two calls for the pairs that start from images (the kinds of defect do not fit into one)."""
    api = _api()
    ctx = api.Kosk(kyber_k=k, max_batch=2)
    checks = ctx.path_count(api.Kosk.PATH_DENSE_CHECK)
    want_checks = 0
    for frm, to in tc.PAIRS:
        for batch in tc.inputs_for(api, k, frm):
            names = [name for name, _ in batch]
            want = [tc.host_transcode(api, k, frm, to, rec) for _, rec in batch]
            st, out = ctx.transcode([rec for _, rec in batch], frm, to)
            where = (k, tc.FMT_NAMES[frm], tc.FMT_NAMES[to], names)
            assert st == [w[0] for w in want], (where, st)
            assert st == [tc.expected_status(frm, to, name) for name in names], (where, st)
            for b in range(5):
                assert len(out[b]) == api.format_bytes(k, to)
                if st[b] < 0:
                    assert out[b] == bytes(len(out[b])), (where, b, "a refused record is not all zero")
                else:
                    assert out[b] == want[b][1], (where, b, _first_diff(out[b], want[b][1]))
            want_checks += 3 if to == tc.FMT_DENSE else 0
    assert ctx.path_count(api.Kosk.PATH_DENSE_CHECK) == checks + want_checks
    # identities on status-0 records
    imgs = tc.image_cases(k)
    good = [imgs["ok"], imgs["ok2"], imgs["ok_big"]]
    st, recs = ctx.transcode(good, api.FMT_IMAGE, api.FMT_DENSE)
    assert st == [0, 0, 0]
    st, back = ctx.transcode(recs, api.FMT_DENSE, api.FMT_IMAGE)
    assert st == [0, 0, 0]
    # (a kept value in [q, 4095] survives; the refilled rows are canonical, as they were in the images)
    assert back == good, [_first_diff(a, b) for a, b in zip(back, good)]
    st, again = ctx.transcode(back, api.FMT_IMAGE, api.FMT_DENSE)
    assert st == [0, 0, 0] and again == recs
    st, comp = ctx.transcode(recs, api.FMT_DENSE, api.FMT_COMPACT)
    assert st == [0, 0, 0]
    assert ctx.transcode(comp, api.FMT_COMPACT, api.FMT_DENSE) == ([0, 0, 0], recs)
    assert ctx.transcode(comp, api.FMT_COMPACT, api.FMT_IMAGE) == ([0, 0, 0], good)
    ctx.close()


# ---- 3. buffers
class _Buf:
    """n records with GUARD bytes of 0xA5 on either side, in pageable memory, kosk_host_alloc memory or device memory at an odd offset"""
    def __init__(self, kind, size, torch, lib):
        self.kind, self.size, self.lib = kind, size, lib
        whole = GUARD + size + GUARD
        if kind == "pageable":
            self.keep = C.create_string_buffer(whole)
            self.base = C.addressof(self.keep)
        elif kind == "pinned":
            self.base = lib.kosk_host_alloc(whole)
            assert self.base
        else:
            self.keep = torch.empty(whole + 16, dtype=torch.uint8, device="cuda")
            self.base = self.keep.data_ptr() + 2
            assert self.base % 16 == 2
        self.ptr = self.base + GUARD
        self.write(b"\xA5" * whole, at=0)

    def write(self, data, at=GUARD):
        if self.kind == "device":
            import torch
            self.keep[2 + at:2 + at + len(data)] = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
            torch.cuda.synchronize()
        else:
            C.memmove(self.base + at, data, len(data))

    def read(self):
        """-> (guard in front, records, guard behind)"""
        whole = GUARD + self.size + GUARD
        raw = self.keep[2:2 + whole].cpu().numpy().tobytes() if self.kind == "device" else C.string_at(self.base, whole)
        return raw[:GUARD], raw[GUARD:GUARD + self.size], raw[GUARD + self.size:]

    def free(self):
        if self.kind == "pinned":
            self.lib.kosk_host_free(C.c_void_p(self.base))


@pytest.mark.parametrize("k", KS)
def test_buffers_pageable_pinned_and_device(k, torch):
    """the same n = 3 batch (max_batch 2: two chunks) image -> dense and dense -> image with `in` and `out` in pageable memory, in
    kosk_host_alloc memory and in device memory at base + 2 bytes, all nine combinations of the first and three of the second: identical
    results, the guard bytes around `out` and the status entries around the n written ones unchanged"""
    api = _api()
    lib = api.lib
    ctx = api.Kosk(kyber_k=k, max_batch=2)
    imgs = tc.image_cases(k)
    n = 3
    legs = []
    batch = [imgs["ok"], imgs["dropped_big"], imgs["kept_big"]]
    want = [tc.host_transcode(api, k, tc.FMT_IMAGE, tc.FMT_DENSE, r) for r in batch]
    assert [w[0] for w in want] == [0, -2, -1]
    legs.append((tc.FMT_IMAGE, tc.FMT_DENSE, batch, want, [(a, b) for a in ("pageable", "pinned", "device") for b in ("pageable", "pinned", "device")]))
    recs = dict(tc.inputs_for(api, k, tc.FMT_DENSE)[0])
    batch = [recs["ok"], recs["dup_I"], recs["ok2"]]
    want = [tc.host_transcode(api, k, tc.FMT_DENSE, tc.FMT_IMAGE, r) for r in batch]
    assert [w[0] for w in want] == [0, 1, 0]
    legs.append((tc.FMT_DENSE, tc.FMT_IMAGE, batch, want, [("pageable", "device"), ("device", "pinned"), ("pinned", "pageable")]))
    for frm, to, batch, want, kinds in legs:
        ib, ob = api.format_bytes(k, frm), api.format_bytes(k, to)
        want_out = b"".join(w[1] if w[0] >= 0 else bytes(ob) for w in want)
        bufs = {}
        for kind in ("pageable", "pinned", "device"):
            bufs["in", kind] = _Buf(kind, n * ib, torch, lib)
            bufs["in", kind].write(b"".join(batch))
            bufs["out", kind] = _Buf(kind, n * ob, torch, lib)
        for kin, kout in kinds:
            src, dst = bufs["in", kin], bufs["out", kout]
            dst.write(b"\x5A" * (n * ob))
            st = (C.c_int32 * (n + 2))(*([77] * (n + 2)))
            rc = lib.kosk_transcode_batch(ctx.handle, n, frm, C.c_void_p(src.ptr), to, C.c_void_p(dst.ptr), C.byref(st, 4))
            assert rc == 0, lib.kosk_last_error(ctx.handle)
            assert list(st) == [77] + [w[0] for w in want] + [77], (k, kin, kout, list(st))
            front, got, behind = dst.read()
            assert front == b"\xA5" * GUARD and behind == b"\xA5" * GUARD, (k, kin, kout, "guard bytes around out")
            assert got == want_out, (k, kin, kout, _first_diff(got, want_out))
            assert src.read() == (b"\xA5" * GUARD, b"".join(batch), b"\xA5" * GUARD), (k, kin, kout, "the input changed")
        for b in bufs.values():
            b.free()
    ctx.close()


# ---- 4. nothing resident moves
def test_resident_state_is_untouched(oracle, torch):
    api = _api()
    k, n = 3, 2
    tapes = [oracle.tape_bytes_for(k, 280 + i) for i in range(n)]
    coins = [hashlib.sha3_256(b"kosk-transcode-test-coins:%d" % b).digest() for b in range(n)]
    ctx = api.Kosk(kyber_k=k, max_batch=n)
    pks, sks, pis = ctx.verifiable_keygen(tapes)
    assert ctx.verify_resident_pk(n) == [True] * n

    def snapshot():
        return (ctx.fetch_proofs(n), ctx.fetch_proofs_dense(n), ctx.verify_resident_pk(n), ctx.fail_masks(n), ctx.kem_enc_verified(n, coins))
    first = snapshot()
    assert first[0] == pis and first[4][2] == [True] * n
    imgs = tc.image_cases(k)
    for frm, to in tc.PAIRS:
        batch = tc.inputs_for(api, k, frm)[0][:3]
        st, out = ctx.transcode([rec for _, rec in batch], frm, to)
        assert st == [tc.expected_status(frm, to, name) for name, _ in batch]
        # (no fetch, no verify in between: the encapsulation must still be armed by the verify call in front of the transcode)
        cts, sss, done = ctx.kem_enc_verified(n, coins)
        assert (cts, sss, done) == first[4], (tc.FMT_NAMES[frm], tc.FMT_NAMES[to])
        assert snapshot() == first, (tc.FMT_NAMES[frm], tc.FMT_NAMES[to])
    # the handle's own proofs through the checking route equal the unchecked pack
    st, recs = ctx.transcode(pis, api.FMT_IMAGE, api.FMT_DENSE)
    assert st == [0] * n and recs == first[1]
    assert ctx.transcode(recs, api.FMT_DENSE, api.FMT_IMAGE) == ([0] * n, pis)
    assert imgs["ok"] != pis[0]
    ctx.close()


# ---- 5. argument errors
def test_argument_errors_leave_the_handle_usable(torch):
    api = _api()
    lib = api.lib
    k = 2
    ctx = api.Kosk(kyber_k=k, max_batch=2)
    h = ctx.handle
    img = tc.image_cases(k)["ok"]
    ib, ob = api.format_bytes(k, 0), api.format_bytes(k, 2)
    src = C.create_string_buffer(img, ib)
    dst = C.create_string_buffer(ib)
    st = (C.c_int32 * 2)(55, 55)
    launches = ctx.path_count(api.Kosk.PATH_DENSE_CHECK)

    def refused(*args):
        assert lib.kosk_transcode_batch(h, *args) == -1
        text = lib.kosk_last_error(h)
        assert text.startswith(b"kosk_transcode_batch: "), text
        return text
    assert b"same format" in refused(1, 0, src, 0, dst, st)
    assert b"same format" in refused(1, 2, src, 2, dst, st)
    for frm, to in ((3, 0), (0, 3), (-1, 2), (0, -1)):
        assert b"format" in refused(1, frm, src, to, dst, st)
    assert b"n must be" in refused(0, 0, src, 2, dst, st)
    assert b"n must be" in refused(-4, 0, src, 2, dst, st)
    assert b"null" in refused(1, 0, None, 2, dst, st)
    assert b"null" in refused(1, 0, src, 2, None, st)
    assert b"null" in refused(1, 0, src, 2, dst, None)
    d = torch.zeros(2 * ib + 64, dtype=torch.uint8, device="cuda")
    p = d.data_ptr()
    assert b"overlap" in refused(1, 0, C.c_void_p(p), 2, C.c_void_p(p + ib - 1), st)           # out starts on the last byte of in
    assert b"overlap" in refused(1, 0, C.c_void_p(p + ob - 1), 2, C.c_void_p(p), st)           # in starts on the last byte of out
    assert b"overlap" in refused(2, 2, C.c_void_p(p + 16), 0, C.c_void_p(p), st)
    assert b"overlap" in refused(1, 0, src, 2, C.cast(src, C.c_void_p), st)
    torch.cuda.synchronize()
    assert list(st) == [55, 55] and dst.raw == bytes(ib) and int(d.sum().item()) == 0, "a refused call started something"
    assert ctx.path_count(api.Kosk.PATH_DENSE_CHECK) == launches
    assert lib.kosk_dense_check_device(h, 0, C.c_void_p(p), (ib + 15) // 16 * 16, C.c_void_p(p)) == -1
    assert lib.kosk_dense_check_device(h, 1, None, (ib + 15) // 16 * 16, C.c_void_p(p)) == -1
    assert lib.kosk_dense_check_device(h, 1, C.c_void_p(p), (ib + 15) // 16 * 16, None) == -1
    # adjacent, not overlapping, is served; and the handle works
    d[:ib] = torch.frombuffer(bytearray(img), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    assert lib.kosk_transcode_batch(h, 1, 0, C.c_void_p(p), 2, C.c_void_p(p + ib), st) == 0 and st[0] == 0
    want = tc.host_transcode(api, k, 0, 2, img)
    assert d[ib:ib + ob].cpu().numpy().tobytes() == want[1]
    assert ctx.transcode([img], api.FMT_IMAGE, api.FMT_DENSE) == ([0], [want[1]])
    ctx.close()


# ---- 6. the workspace is in the inventory, as public buffers
def test_workspace_is_in_the_inventory_as_public(torch):
    api = _api()
    k = 2
    ctx = api.Kosk(kyber_k=k, max_batch=2)
    img = tc.image_cases(k)["ok"]
    needle = img[5000:5032]
    assert ctx.secret_scan(needle) == 0
    st, recs = ctx.transcode([img], api.FMT_IMAGE, api.FMT_DENSE)
    assert st == [0]
    hits = ctx.secret_scan(needle)
    assert hits >= 1, "the transcoder's workspace is not in the buffer inventory"
    ctx.wipe_secrets()
    assert ctx.secret_scan(needle) == hits, "a wipe cleared public buffers of the transcoder (or they are filed as secret)"
    assert ctx.transcode(recs, api.FMT_DENSE, api.FMT_IMAGE) == ([0], [img])
    ctx.close()   # kosk_destroy frees the workspace with everything else in the inventory
