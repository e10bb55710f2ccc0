"""Inputs and expected results shared by tests/test_dense2_host.py and tests/test_gpu_30_dense2.py (kosk-dense-v2).
The references are the numpy model tests/dense2_model.py and, for whole records, the composition of the host codecs (which the host test
pins to that model).  Results are computed once and shared."""
import ctypes as C
import functools
import hashlib

import numpy as np

from tests import dense2_model as d2
from tests import opened_sets

FMT_IMAGE, FMT_COMPACT, FMT_DENSE, FMT_DENSE2 = 0, 1, 2, 4
FMTS = (FMT_IMAGE, FMT_COMPACT, FMT_DENSE, FMT_DENSE2)
PAIRS = [(a, b) for a in FMTS for b in FMTS if a != b]
FMT_NAMES = {0: "image", 1: "compact", 2: "dense", 4: "dense2"}


@functools.lru_cache(maxsize=None)
def oracle_proof(k):
    from tests import oracle_lib
    return oracle_lib.verifiable_keygen(k, oracle_lib.tape_bytes_for(k, 0))[2]


def get16(img, off):
    return img[off] | (img[off + 1] << 8)


def put16(img, off, v):
    img[off] = v & 0xFF
    img[off + 1] = v >> 8


def at(k, f, row, col=0):
    """image offset of u16 (row, col) of a truncated field; col < 0 counts from the end of the row"""
    off, _size, cols = d2.field_table(k)[0][f]
    return off + 2 * (row * cols + (col if col >= 0 else cols + col))


# ---- synthetic images for the kernel-level calls
def opened_lists(rng):
    """both ends, across a gap, every third party, random, and a duplicated entry (tests/opened_sets.py)"""
    cat = opened_sets.CATALOGUE
    rand = rng.permutation(d2.NPARTY)[:d2.NOPEN].tolist()
    dup = rng.permutation(d2.NPARTY)[:d2.NOPEN].tolist()
    dup[140] = dup[2]
    return {"first150": cat["first150"], "last150": cat["last150"], "gap": cat["above_points"], "third": cat["every_third"],
            "random": rand, "dup": dup}


def synthetic(k, rng, opened, big=False):
    """an image whose u16 are random below q (kept rows of the nine fields optionally with values in [q, 4095], the first and the last kept
    value 4095); the dropped rows are garbage until refill() has run"""
    tab, total = d2.field_table(k)
    img = bytearray(rng.integers(0, d2.Q, size=total // 2, dtype=np.uint16).tobytes())
    img[tab[d2.F_I][0]:tab[d2.F_I][0] + 2 * d2.NOPEN] = np.array(opened, np.uint16).tobytes()
    if big:
        for f in d2.LISTED:
            off, size, cols = tab[f]
            nb = d2.ROWS[f] * cols * 2
            v = np.frombuffer(bytes(img[off:off + nb]), np.uint16).copy()
            sel = rng.random(len(v)) < 0.25
            v[sel] = rng.integers(d2.Q, 4096, size=int(sel.sum()), dtype=np.uint16)
            v[0], v[-1] = 4095, 4095
            img[off:off + nb] = v.tobytes()
    return img


_refills = {}


def model_check(k, img):
    """what kosk_dense2_check_device must say, by the model: 1 a malformed I; 2 a dropped row is not the refill of the kept ones; else 0.
    The refill depends on I and the kept rows only and is computed once per such input."""
    tab, _ = d2.field_table(k)
    img = bytes(img)
    opened = np.frombuffer(img[tab[d2.F_I][0]:tab[d2.F_I][0] + 2 * d2.NOPEN], np.uint16)
    if d2.malformed(opened):
        return 1
    kept = lambda x: b"".join(x[tab[f][0]:tab[f][0] + d2.ROWS[f] * tab[f][2] * 2] for f in d2.LISTED)
    dropped = lambda x: b"".join(x[tab[f][0] + d2.ROWS[f] * tab[f][2] * 2:tab[f][0] + tab[f][1]] for f in d2.LISTED)
    key = hashlib.sha256(opened.tobytes() + kept(img)).digest()
    if key not in _refills:
        w = bytearray(img)
        assert d2.refill(k, w) == 0
        _refills[key] = dropped(bytes(w))
    return 0 if _refills[key] == dropped(img) else 2


def check_mutations(k, img):
    """[(what, offset, new u16, status the issue states or None where the model decides)] on a representable image: the first u16 of row R
    and the last of row 1303 of all nine fields, v + q, 0xFFFF, a kept value at row R - 1, and the u16 on either side of every field"""
    tab, _ = d2.field_table(k)
    out = []
    for f in d2.LISTED:
        R = d2.ROWS[f]
        for what, off in (("first u16 of row %d" % R, at(k, f, R, 0)), ("last u16 of row 1303", at(k, f, d2.NREST - 1, -1))):
            out.append(("%s of field %d" % (what, f), off, (get16(img, off) + 1) % d2.Q, 2))
    off = at(k, 21, 900, 0)
    while get16(img, off) + d2.Q >= 4096:
        off += 2
    out.append(("v + q in a dropped row of field 21", off, get16(img, off) + d2.Q, 2))
    out.append(("0xFFFF in a dropped row of field 16", at(k, 16, 152, 1), 0xFFFF, 2))
    for f in (15, 22):
        off = at(k, f, d2.ROWS[f] - 1, -1)
        out.append(("last u16 of row R - 1 of field %d" % f, off, (get16(img, off) + 1) % d2.Q, 2))
    for f in d2.LISTED:
        for what, off in (("first u16 behind field %d" % f, tab[f + 1][0]), ("last u16 in front of field %d" % f, tab[f][0] - 2)):
            out.append((what, off, get16(img, off) ^ 1, None))
    return out


# ---- whole records: the host codecs' composition
def _decode(api, k, fmt, rec):
    if fmt == FMT_IMAGE:
        return 0, rec
    if fmt == FMT_COMPACT:
        out = C.create_string_buffer(api.proof_bytes(k))
        assert api.lib.kosk_proof_decompress(k, rec, out) == 0
        return 0, out.raw
    return api.dense_unpack(k, rec) if fmt == FMT_DENSE else api.proof_dense2_unpack(k, rec)


def _encode(api, k, fmt, img):
    if fmt == FMT_IMAGE:
        return 0, img
    if fmt == FMT_COMPACT:
        out = C.create_string_buffer(api.lib.kosk_compact_proof_bytes(k))
        return api.lib.kosk_proof_compress(k, img, out), out.raw
    return api.dense_pack(k, img) if fmt == FMT_DENSE else api.proof_dense2_pack(k, img)


_host = {}


def host_transcode(api, k, frm, to, rec):
    """(status, record or None): the encoder's result if it is nonzero, otherwise the decoder's"""
    key = (k, frm, to, hashlib.sha256(rec).digest())
    if key not in _host:
        dec, img = _decode(api, k, frm, rec)
        enc, out = _encode(api, k, to, img)
        _host[key] = ((enc if enc else dec), (out if enc >= 0 else None))
    return _host[key]


@functools.lru_cache(maxsize=None)
def transcode_images(k):
    """{name: (image, status to compact, to dense, to dense2)}: the kinds of image the formats tell apart, made from the oracle's proof"""
    pi = oracle_proof(k)
    tab, _ = d2.field_table(k)
    out = {"ok": (pi, 0, 0, 0)}

    def edit(name, off, v, *status):
        img = bytearray(pi)
        put16(img, off, v)
        out[name] = (bytes(img),) + status
    edit("kept_big", at(k, 15, 10, 0), 4096, -1, -1, -1)                        # a row all three store
    edit("eta_row300_big", at(k, 15, 300, 0), 4096, -1, -1, -2)                 # stored by v1, dropped by v2
    edit("u_row900_big", at(k, 21, 900, 0), 4096, -1, -1, -2)                   # field 21: whole in v1, dropped by v2
    off = at(k, 22, 1000, 1)
    edit("u_row1000_changed", off, (get16(pi, off) + 1) % d2.Q, 0, 0, -2)
    off = at(k, 8, 1000, 0)
    edit("t_row1000_changed", off, (get16(pi, off) + 1) % d2.Q, 0, -2, -2)
    off, size, cols = tab[16]
    v = np.frombuffer(pi[off:off + size], np.uint16).reshape(d2.NREST, cols).astype(np.int64)
    v[:, 1] = (v[:, 1] + 1) % d2.Q                                              # degree <= 406 still, other values at the packed positions
    out["eta_other_secret"] = (pi[:off] + v.astype(np.uint16).tobytes() + pi[off + size:], 0, 0, -2)
    oi = tab[d2.F_I][0]
    edit("bad_I", oi + 2 * 140, get16(pi, oi + 4), 0, -2, -2)
    return out


def bad_I_record(k, rec, layout, kind):
    """the record with its opened list made malformed: kind "dup" or "range" """
    ro, rb = layout[d2.F_I]
    opened = d2.unpack12(bytes(rec[ro:ro + rb]), d2.NOPEN)
    if kind == "dup":
        opened[9] = opened[100]
    else:
        opened[33] = d2.NPARTY
    r = bytearray(rec)
    r[ro:ro + rb] = d2.pack12(opened).tobytes()
    return bytes(r)
