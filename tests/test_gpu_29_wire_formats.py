"""The three wire formats (image, compact, dense) through the same calls: host-buffer key generation and verification by format and
randomness source, the resident fetch / stage calls, page-locked buffers, and what every entry point answers at n = 0 and
n = max_batch + 1.  Public API only; K = 2, a handle of max_batch 2 and n = 3 proofs (two chunks, the second ragged)."""
import ctypes as C

import pytest

pytestmark = pytest.mark.gpu

K, CAP, N = 2, 2, 3
FORMATS = ["image", "compact", "dense"]
F_COMM = 23  # the view-commitment digests: raw bytes in all three formats


@pytest.fixture(scope="module")
def torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return torch


def _api():
    from mpcith_kyber_kosk_amd import api
    return api


def _fns(lib, fmt):
    sfx = {"image": "", "compact": "_compact", "dense": "_dense"}[fmt]
    return {"tapes": getattr(lib, "kosk_verifiable_keygen_batch" + sfx), "seeds": getattr(lib, "kosk_verifiable_keygen_seeded_batch" + sfx),
            "verify": getattr(lib, "kosk_verify_batch" + sfx), "fetch": getattr(lib, "kosk_fetch_proofs" + sfx),
            "stage": getattr(lib, "kosk_stage_verifier_inputs" + sfx)}


def _size(api, fmt):
    return api.format_bytes(K, FORMATS.index(fmt))


def _encode(api, fmt, img):
    """the host codec of `fmt` on one image"""
    if fmt == "image":
        return img
    out = C.create_string_buffer(_size(api, fmt))
    fn = api.lib.kosk_proof_compress if fmt == "compact" else api.lib.kosk_proof_dense_pack
    assert fn(K, C.c_char_p(img), out) == 0
    return out.raw


class _Room:
    """n records of `size` bytes in pageable or kosk_host_alloc memory"""

    def __init__(self, lib, nbytes, pinned):
        self.lib, self.nbytes, self.pinned = lib, nbytes, pinned
        if pinned:
            self.ptr = lib.kosk_host_alloc(nbytes)
            assert self.ptr
        else:
            self.buf = C.create_string_buffer(nbytes)
            self.ptr = C.addressof(self.buf)
        self.arg = C.c_void_p(self.ptr)

    def raw(self):
        return C.string_at(self.ptr, self.nbytes)

    def put(self, data):
        C.memmove(self.ptr, data, len(data))

    def free(self):
        if self.pinned:
            self.lib.kosk_host_free(C.c_void_p(self.ptr))


def _keygen(api, ctx, fmt, source, rand, pinned=False):
    """the host-buffer key generation of `fmt` through lib -> (pk, sk, records), each the whole buffer"""
    lib = api.lib
    pk = C.create_string_buffer(ctx.pk_bytes * N); sk = C.create_string_buffer(ctx.sk_bytes * N)
    room = _Room(lib, _size(api, fmt) * N, pinned)
    stride = ctx.tape_bytes if source == "tapes" else api.SEED_BYTES
    assert _fns(lib, fmt)[source](ctx.handle, N, C.c_char_p(b"".join(rand)), stride, pk, sk, room.arg) == 0, lib.kosk_last_error(ctx.handle)
    out = room.raw()
    room.free()
    return pk.raw, sk.raw, out


def _verify(api, ctx, fmt, recs, pk, pinned=False):
    lib = api.lib
    room = _Room(lib, len(recs), pinned)
    room.put(recs)
    ok = C.create_string_buffer(N)
    assert _fns(lib, fmt)["verify"](ctx.handle, N, room.arg, C.c_char_p(pk), ok) == 0
    room.free()
    return ok.raw, ctx.fail_masks(N)


@pytest.fixture(scope="module")
def base(oracle, torch):
    """the image calls of both sources, computed once and left unchanged"""
    api = _api()
    ctx = api.Kosk(kyber_k=K, max_batch=CAP)
    rand = {"tapes": [oracle.tape_bytes_for(K, 70 + i) for i in range(N)], "seeds": [bytes([0x29, i]) * 16 for i in range(N)]}
    img = {src: _keygen(api, ctx, "image", src, rand[src]) for src in ("tapes", "seeds")}
    yield api, ctx, rand, img
    ctx.close()


def test_seeded_image_call_is_the_tape_call_on_expanded_tapes(base):
    api, ctx, rand, img = base
    tapes = [api.tape_from_seed(K, s) for s in rand["seeds"]]
    assert _keygen(api, ctx, "image", "tapes", tapes) == img["seeds"]


@pytest.mark.parametrize("source", ["tapes", "seeds"])
@pytest.mark.parametrize("fmt", FORMATS)
def test_keygen_by_format_and_source(base, fmt, source):
    api, ctx, rand, img = base
    pk0, sk0, pi0 = img[source]
    pb = ctx.proof_bytes
    want = b"".join(_encode(api, fmt, pi0[b * pb:(b + 1) * pb]) for b in range(N))
    pk, sk, recs = _keygen(api, ctx, fmt, source, rand[source])
    assert pk == pk0 and sk == sk0
    assert recs == want, "the records of the %s call differ from the host codec of the image call's proofs" % fmt


def _tampered(api, ctx, pi0):
    """records of all three formats for the image call's proofs with one bit of proof 2 flipped in a field every format stores raw"""
    pb = ctx.proof_bytes
    imgs = [pi0[b * pb:(b + 1) * pb] for b in range(N)]
    bad = bytearray(imgs[2]); bad[api.proof_field(K, F_COMM)[0] + 5] ^= 0x04
    imgs[2] = bytes(bad)
    return {fmt: b"".join(_encode(api, fmt, im) for im in imgs) for fmt in FORMATS}


def test_verify_by_format(base):
    api, ctx, rand, img = base
    pk0, _sk0, pi0 = img["tapes"]
    pb = ctx.proof_bytes
    bad = _tampered(api, ctx, pi0)
    masks = {}
    for fmt in FORMATS:
        good = b"".join(_encode(api, fmt, pi0[b * pb:(b + 1) * pb]) for b in range(N))
        ok, m = _verify(api, ctx, fmt, good, pk0)
        assert ok == b"\x01\x01\x01" and m == [0, 0, 0], fmt
        ok, masks[fmt] = _verify(api, ctx, fmt, bad[fmt], pk0)
        assert ok == b"\x01\x01\x00", fmt
    assert masks["image"][:2] == [0, 0] and masks["image"][2] != 0
    assert masks["compact"] == masks["image"] and masks["dense"] == masks["image"]


def test_resident_calls(base):
    api, _ctx, rand, img = base
    n = 2
    ctx = api.Kosk(kyber_k=K, max_batch=CAP)
    assert ctx.verifiable_keygen_resident(rand["tapes"][:n]) == n
    pks, _sks = ctx.keys(n)
    pb = ctx.proof_bytes
    got = {"image": ctx.fetch_proofs(n), "compact": ctx.fetch_proofs_compact(n), "dense": ctx.fetch_proofs_dense(n)}
    pis = got["image"]
    assert b"".join(pks) == img["tapes"][0][:n * ctx.pk_bytes] and b"".join(pis) == img["tapes"][2][:n * pb]
    for fmt in FORMATS:
        assert got[fmt] == [_encode(api, fmt, pi) for pi in pis], fmt
    ver = api.Kosk(kyber_k=K, max_batch=CAP)
    stage = {"image": ver.stage_verifier_inputs, "compact": ver.stage_verifier_inputs_compact, "dense": ver.stage_verifier_inputs_dense}
    for fmt in FORMATS:
        stage[fmt](got[fmt], pks)
        assert ver.verify_resident(n) == [True] * n, fmt
        assert ver.fetch_proofs(n) == pis, fmt
    ctx.close(); ver.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_pinned_buffers(base, fmt):
    api, _ctx, rand, img = base
    pk0, sk0, pi0 = img["tapes"]
    ctx = api.Kosk(kyber_k=K, max_batch=CAP)
    pageable = _keygen(api, ctx, fmt, "tapes", rand["tapes"])
    pc0 = ctx.path_counts()
    pinned = _keygen(api, ctx, fmt, "tapes", rand["tapes"], pinned=True)
    assert pinned == pageable and pinned[:2] == (pk0, sk0)
    pc1 = ctx.path_counts()
    assert pc1["copy_direct"] == pc0["copy_direct"] + 2 and pc1["copy_staged"] == pc0["copy_staged"]   # one record copy per chunk
    bad = _tampered(api, ctx, pi0)[fmt]
    for recs, want in ((pinned[2], b"\x01\x01\x01"), (bad, b"\x01\x01\x00")):
        ok_pageable = _verify(api, ctx, fmt, recs, pk0)
        pc0 = ctx.path_counts()
        ok_pinned = _verify(api, ctx, fmt, recs, pk0, pinned=True)
        pc1 = ctx.path_counts()
        assert ok_pinned == ok_pageable and ok_pinned[0] == want
        assert pc1["copy_direct"] == pc0["copy_direct"] + 2 and pc1["copy_staged"] == pc0["copy_staged"]
    ctx.close()


def test_edge_calls(base):
    """n = 0 on every host-buffer and resident entry point of the three formats, n = max_batch + 1 on the resident ones: the
    return values and the state of the fail masks as the calls have always answered (wire formats as a parameter)"""
    api, _ctx, rand, img = base
    lib = api.lib
    pk0, _sk0, pi0 = img["tapes"]
    ctx = api.Kosk(kyber_k=K, max_batch=CAP)
    h = ctx.handle
    pk = C.create_string_buffer(ctx.pk_bytes * N); sk = C.create_string_buffer(ctx.sk_bytes * N); ok = C.create_string_buffer(N)
    m = (C.c_uint32 * N)()
    pb = ctx.proof_bytes
    for fmt in FORMATS:
        fns = _fns(lib, fmt)
        room = C.create_string_buffer(_size(api, fmt) * N)
        # key generation at n = 0: nothing to do, 0
        assert fns["tapes"](h, 0, C.c_char_p(b"".join(rand["tapes"])), ctx.tape_bytes, pk, sk, room) == 0, fmt
        assert fns["seeds"](h, 0, C.c_char_p(b"".join(rand["seeds"])), api.SEED_BYTES, pk, sk, room) == 0, fmt
        # verification at n = 0: 0, and the masks of the call before are gone
        good = b"".join(_encode(api, fmt, pi0[b * pb:(b + 1) * pb]) for b in range(N))
        assert _verify(api, ctx, fmt, good, pk0)[0] == b"\x01\x01\x01"
        assert lib.kosk_verify_fail_masks(h, m, N) == 0
        assert fns["verify"](h, 0, room, pk, ok) == 0, fmt
        assert lib.kosk_verify_fail_masks(h, m, 1) == -1 and lib.kosk_verify_fail_masks(h, m, 0) == 0, fmt
        # the resident calls at n = 0: the image ones refuse, the packed ones have nothing to do; none touches the masks
        assert _verify(api, ctx, fmt, good, pk0)[0] == b"\x01\x01\x01"
        want = -1 if fmt == "image" else 0
        assert fns["fetch"](h, 0, room) == want, fmt
        if want:
            assert b"kosk_fetch_proofs: invalid argument" in lib.kosk_last_error(h)
        assert fns["stage"](h, 0, room, pk) == want, fmt
        if want:
            assert b"kosk_stage_verifier_inputs: invalid argument" in lib.kosk_last_error(h)
        # ... and at n = max_batch + 1: refused, whatever the format
        sfx = {"image": "", "compact": "_compact", "dense": "_dense"}[fmt]
        assert fns["fetch"](h, CAP + 1, room) == -1, fmt
        assert ("kosk_fetch_proofs%s: invalid argument" % sfx).encode() in lib.kosk_last_error(h)
        assert fns["stage"](h, CAP + 1, room, pk) == -1, fmt
        assert ("kosk_stage_verifier_inputs%s: invalid argument" % sfx).encode() in lib.kosk_last_error(h)
        assert lib.kosk_verify_fail_masks(h, m, N) == 0 and list(m) == [0, 0, 0], fmt
    ctx.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_short_tape_is_refused_in_every_format(base, fmt):
    """the binding's check of the image call holds for all three formats (the one behaviour this file pins that the compact and dense
    methods did not have before they shared a body with the image one)"""
    api, ctx, rand, _img = base
    call = {"image": ctx.verifiable_keygen, "compact": ctx.verifiable_keygen_compact, "dense": ctx.verifiable_keygen_dense}[fmt]
    with pytest.raises(api.KoskError, match="tape shorter than kosk_tape_bytes"):
        call([rand["tapes"][0], rand["tapes"][1][:-1]])
