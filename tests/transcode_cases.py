"""Inputs and expected results of the transcoding tests (kosk_transcode_batch, kosk_dense_check_device), shared by
tests/test_transcode_host.py (which holds the expected statuses to the numpy model tests/dense_model.py) and tests/test_gpu_28_transcode.py
(which holds the GPU to the host codecs).  Everything is synthetic -- random u16 below q, a chosen opened list, rows 407..1303 of the listed
fields made representable by dense_model.refill -- so no prover is needed.  Results are computed once per K and shared."""
import ctypes as C
import functools
import hashlib

import numpy as np

from tests import dense_model as dm

KS = (2, 3, 4)
FMT_IMAGE, FMT_COMPACT, FMT_DENSE = 0, 1, 2
FMT_NAMES = {FMT_IMAGE: "image", FMT_COMPACT: "compact", FMT_DENSE: "dense"}
PAIRS = [(a, b) for a in (FMT_IMAGE, FMT_COMPACT, FMT_DENSE) for b in (FMT_IMAGE, FMT_COMPACT, FMT_DENSE) if a != b]


# ---- images
def opened_sets(rng):
    """the six opened sets of tests/test_gpu_19_dense.py"""
    third = list(range(0, 3 * dm.NOPEN, 3))
    rand = rng.permutation(dm.NPARTY)[:dm.NOPEN].tolist()
    dup = rng.permutation(dm.NPARTY)[:dm.NOPEN].tolist()
    dup[140] = dup[2]
    return {"low": list(range(dm.NOPEN)), "high": list(range(dm.NREST, dm.NPARTY)), "gap": list(range(257, 407)), "third": third,
            "random": rand, "dup": dup}


def synthetic(k, rng, opened, big=False):
    """an image whose u16 are random below q (kept rows of the listed fields optionally with values in [q, 4095]); rows 407..1303 of the
    listed fields are garbage until refill() has run"""
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


def get16(img, off):
    return img[off] | (img[off + 1] << 8)


def put16(img, off, v):
    img[off] = v & 0xFF
    img[off + 1] = v >> 8


def row_off(k, f, row, col=0):
    """image offset of u16 (row, col) of listed field f; col < 0 counts from the end of the row"""
    off, size, cols = dm.field_table(k)[0][f]
    return off + 2 * (row * cols + (col if col >= 0 else cols + col))


_refills = {}


def model_check(k, img):
    """what kosk_dense_check_device must say about an image, by the model: 1 a malformed I; 2 rows 407..1303 of a listed field are not
    dense_model.refill of rows 0..406; else 0.  The refill depends on I and the kept rows only and is kept per such input."""
    tab, _ = dm.field_table(k)
    img = bytes(img)
    opened = np.frombuffer(img[tab[dm.F_I][0]:tab[dm.F_I][0] + 2 * dm.NOPEN], np.uint16)
    if dm.malformed(opened):
        return 1
    dropped = lambda x: b"".join(x[tab[f][0] + dm.KEPT * tab[f][2] * 2:tab[f][0] + tab[f][1]] for f in dm.LISTED)
    key = hashlib.sha256(opened.tobytes() + b"".join(img[tab[f][0]:tab[f][0] + dm.KEPT * tab[f][2] * 2] for f in dm.LISTED)).digest()
    if key not in _refills:
        w = bytearray(img)
        assert dm.refill(k, w) == 0
        _refills[key] = dropped(bytes(w))
    return 0 if _refills[key] == dropped(img) else 2


def check_mutations(k, img):
    """[(what, offset, new u16, status the issue states or None where only the model decides)]: one changed u16 each, for an image that
    is representable.  The first u16 of row 407 and the last of row 1303 of every listed field, v + q and 0xFFFF in the middle, a kept
    value (the last u16 of row 406), and the u16 on either side of every listed field: those share a 16-byte chunk with filled rows and
    must not be taken for them -- status 0, unless the neighbour is itself a listed field, where the changed u16 is a kept value (the
    field behind) or a filled one (the field in front) and the model says 2."""
    tab, _ = dm.field_table(k)
    out = []
    for f in dm.LISTED:
        for what, off in (("first u16 of row 407", row_off(k, f, dm.KEPT, 0)), ("last u16 of row 1303", row_off(k, f, dm.NREST - 1, -1))):
            out.append(("%s of field %d" % (what, f), off, (get16(img, off) + 1) % dm.Q, 2))
    off = congruent_site(k, img, 3)
    out.append(("v + q in the middle of field 3", off, get16(img, off) + dm.Q, 2))
    out.append(("0xFFFF in the middle of field 14", row_off(k, 14, 800, 1), 0xFFFF, 2))
    off = row_off(k, 15, dm.KEPT - 1, -1)
    out.append(("last u16 of row 406 of field 15", off, (get16(img, off) + 1) % dm.Q, 2))
    for f in dm.LISTED:
        for what, off, g in (("first u16 of field %d behind field %d" % (f + 1, f), tab[f + 1][0], f + 1),
                             ("last u16 of field %d in front of field %d" % (f - 1, f), tab[f][0] - 2, f - 1)):
            out.append((what, off, get16(img, off) ^ 1, 2 if g in dm.LISTED else 0))
    return out


# ---- the cases of kosk_transcode_batch
def _middle(k, f):
    return row_off(k, f, 800, 1)


def congruent_site(k, img, f):
    """offset of the first u16 from row 800 on of listed field f whose value v has v + q < 4096"""
    off = row_off(k, f, 800, 0)
    while get16(img, off) + dm.Q >= 4096:
        off += 2
    assert off < row_off(k, f, dm.NREST - 1, 0)
    return off


@functools.lru_cache(maxsize=None)
def image_cases(k):
    """{name: image}: the kinds of defect the call tells apart, one image each"""
    rng = np.random.default_rng(2800 + k)
    sets = opened_sets(rng)
    tab, _ = dm.field_table(k)
    ok = synthetic(k, rng, sets["random"])
    assert dm.refill(k, ok) == 0
    ok2 = synthetic(k, rng, sets["third"])
    assert dm.refill(k, ok2) == 0
    ok_big = synthetic(k, rng, sets["gap"], big=True)      # kept values in [q, 4095]: representable, the refill reduces them
    assert dm.refill(k, ok_big) == 0
    out = {"ok": ok, "ok2": ok2, "ok_big": ok_big}

    def variant(name, base, edits):
        img = bytearray(base)
        for off, v in edits:
            put16(img, off, v)
        out[name] = img
    variant("kept_big", ok, [(row_off(k, 8, 200, 1), 4096)])                  # a stored value >= 4096 in a listed field
    variant("other_big", ok, [(tab[0][0] + 10, 0x8001)])                      # ... in a field that is stored whole
    variant("dropped_big", ok, [(_middle(k, 13), 0xF123)])                    # ... in a dropped row only
    variant("both", ok, [(row_off(k, 2, 0, 0), 5000), (_middle(k, 3), get16(ok, _middle(k, 3)) ^ 1)])
    cong = congruent_site(k, ok2, 2)
    variant("congruent", ok2, [(cong, get16(ok2, cong) + dm.Q)])              # v + q below 4096 in a dropped row
    variant("dropped_small", ok2, [(row_off(k, 16, dm.NREST - 1, -1), (get16(ok2, row_off(k, 16, dm.NREST - 1, -1)) + 1) % dm.Q)])
    bad_I = bytearray(ok)
    put16(bad_I, tab[dm.F_I][0] + 2 * 140, get16(ok, tab[dm.F_I][0] + 4))    # a duplicate; its dropped rows stay those of `ok`
    out["bad_I"] = bad_I
    return {name: bytes(img) for name, img in out.items()}


# name -> (status to dense, status to compact) of an image input, as the issue states them
IMAGE_STATUS = {"ok": (0, 0), "ok2": (0, 0), "ok_big": (0, 0), "kept_big": (-1, -1), "other_big": (-1, -1), "dropped_big": (-2, -1),
                "both": (-1, -1), "congruent": (-2, 0), "dropped_small": (-2, 0), "bad_I": (-2, 0)}
# two calls of n = 5 per pair that starts from images (every kind at some chunk position of a handle of max_batch 2), one for the others
IMAGE_BATCHES = (("ok", "kept_big", "dropped_big", "bad_I", "ok_big"), ("other_big", "both", "ok2", "congruent", "dropped_big"))
COMPACT_BATCH = ("ok", "congruent", "bad_I", "ok_big", "dropped_small")    # images that compress; to dense: 0 -2 -2 0 -2
DENSE_BATCH = ("ok", "dup_I", "ok_big", "range_I", "ok2")                   # records; to image / compact: 0 1 0 1 0
DENSE_STATUS = {"ok": 0, "ok2": 0, "ok_big": 0, "dup_I": 1, "range_I": 1}


def dense_records(k, pack):
    """{name: dense record} of DENSE_BATCH: packed images (pack: image -> record, status 0 asserted by the caller's codec), and two records
    whose opened list was replaced by a malformed one"""
    imgs = image_cases(k)
    out = {name: pack(imgs[name]) for name in ("ok", "ok2", "ok_big")}
    lay, _ = dm.record_layout(k)
    ro, rb = lay[dm.F_I]
    opened = dm.unpack12(out["ok"][ro:ro + rb], dm.NOPEN)
    for name, pos, val in (("dup_I", 9, int(opened[100])), ("range_I", 33, dm.NPARTY)):
        o2 = opened.copy()
        o2[pos] = val
        r = bytearray(out["ok"])
        r[ro:ro + rb] = dm.pack12(o2).tobytes()
        out[name] = bytes(r)
    return out


def compress(api, k, img):
    """kosk_proof_compress -> (return code, record)"""
    out = C.create_string_buffer(api.lib.kosk_compact_proof_bytes(k))
    rc = api.lib.kosk_proof_compress(k, C.c_char_p(bytes(img)), out)
    return rc, out.raw


def decompress(api, k, rec):
    out = C.create_string_buffer(api.proof_bytes(k))
    assert api.lib.kosk_proof_decompress(k, C.c_char_p(bytes(rec)), out) == 0
    return out.raw


_host = {}


def host_transcode(api, k, frm, to, rec):
    """the contract: the host codecs' composition on one record -> (status, output record or None for a negative status)"""
    key = (k, frm, to, hashlib.sha256(rec).digest())
    if key in _host:
        return _host[key]
    dec = 0
    if frm == FMT_IMAGE:
        img = rec
    elif frm == FMT_COMPACT:
        img = decompress(api, k, rec)
    else:
        dec, img = api.dense_unpack(k, rec)
    if to == FMT_IMAGE:
        enc, out = 0, img
    elif to == FMT_COMPACT:
        enc, out = compress(api, k, img)
    else:
        enc, out = api.dense_pack(k, img)
    res = (enc if enc else dec, out if enc >= 0 else None)
    _host[key] = res
    return res


def inputs_for(api, k, frm):
    """[[(name, record)] per call] of the pair's `from` side"""
    imgs = image_cases(k)
    if frm == FMT_IMAGE:
        return [[(name, imgs[name]) for name in batch] for batch in IMAGE_BATCHES]
    if frm == FMT_COMPACT:
        recs = [(name,) + compress(api, k, imgs[name]) for name in COMPACT_BATCH]
        assert all(rc == 0 for _, rc, _ in recs)
        return [[(name, rec) for name, _, rec in recs]]

    def pack(img):
        st, rec = host_transcode(api, k, FMT_IMAGE, FMT_DENSE, img)
        assert st == 0
        return rec
    recs = dense_records(k, pack)
    return [[(name, recs[name]) for name in DENSE_BATCH]]


def expected_status(frm, to, name):
    """the status table as the issue states it, by the name of the input"""
    if frm == FMT_DENSE:
        return DENSE_STATUS[name]
    if to == FMT_IMAGE:
        return 0
    return IMAGE_STATUS[name][0 if to == FMT_DENSE else 1]
