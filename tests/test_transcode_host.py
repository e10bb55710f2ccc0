"""Transcoding between the wire formats, the parts that need no GPU: the names are declared, bound and exported,
kosk_format_bytes, the NULL-argument returns, and the status table that tests/test_gpu_28_transcode.py holds the GPU to -- computed here
with the host codecs AND with the numpy model tests/dense_model.py, which must agree with each other and with the statuses the cases are
named for."""
import ctypes as C
import os
import re

import pytest

from tests import dense_model as dm
from tests import transcode_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kosk_transcode_batch", "kosk_dense_check_device"]


@pytest.fixture(scope="module")
def api():
    from mpcith_kyber_kosk_amd import api
    return api


def test_names_are_declared_bound_and_exported(api):
    header = open(os.path.join(ROOT, "include", "kosk_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(kosk_ctx \*ctx" % name, code), name
    assert re.search(r"\bsize_t kosk_format_bytes\s*\(int kyber_k, int fmt\)", code)
    for name in NAMES + ["kosk_format_bytes"]:
        assert name in api.EXPORTS and hasattr(api.lib, name), name
        assert getattr(api.lib, name).argtypes is not None, name
    assert re.search(r"enum\s*\{\s*KOSK_FMT_IMAGE = 0,\s*KOSK_FMT_COMPACT = 1,\s*KOSK_FMT_DENSE = 2\s*\}", code)
    assert (api.FMT_IMAGE, api.FMT_COMPACT, api.FMT_DENSE) == (0, 1, 2) == (tc.FMT_IMAGE, tc.FMT_COMPACT, tc.FMT_DENSE)
    assert api.Kosk.PATH_DENSE_CHECK == 22
    for method in ("transcode", "dense_check_device"):
        assert callable(getattr(api.Kosk, method))
    assert callable(api.format_bytes)
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int kosk_path_count\(", header, flags=re.S)
    assert m and re.search(r"\b22 launches of k_dense_check\b", m.group(1))


def test_format_bytes(api):
    lib = api.lib
    for k in tc.KS:
        assert lib.kosk_format_bytes(k, 0) == lib.kosk_proof_bytes(k) == dm.image_bytes(k)
        assert lib.kosk_format_bytes(k, 1) == lib.kosk_compact_proof_bytes(k) > 0
        assert lib.kosk_format_bytes(k, 2) == lib.kosk_dense_proof_bytes(k) == dm.dense_bytes(k)
        assert lib.kosk_format_bytes(k, -1) == 0 and lib.kosk_format_bytes(k, 3) == 0
        assert api.format_bytes(k, api.FMT_DENSE) == dm.dense_bytes(k)
    for k in (1, 5):
        assert [lib.kosk_format_bytes(k, f) for f in (0, 1, 2)] == [0, 0, 0]


def test_null_arguments_return_minus_one(api):
    lib = api.lib
    buf = C.create_string_buffer(64)
    st = (C.c_int32 * 1)()
    assert lib.kosk_transcode_batch(None, 1, 0, buf, 2, buf, st) == -1
    assert lib.kosk_dense_check_device(None, 1, buf, 64, buf) == -1


def _model_transcode(k, frm, to, rec, imgs_by_compact):
    """the same composition by the model: dense by dense_model.pack / unpack; the compact codec has no model of its own, so a compact
    record stands for the image it was made from and "to compact" fails exactly on a u16 >= 4096 outside the raw fields"""
    import numpy as np
    dec = 0
    if frm == tc.FMT_IMAGE:
        img = rec
    elif frm == tc.FMT_COMPACT:
        img = imgs_by_compact[rec]
    else:
        dec, img = dm.unpack(k, rec)
    if to == tc.FMT_IMAGE:
        enc = 0
    elif to == tc.FMT_COMPACT:
        tab, _ = dm.field_table(k)
        enc = -1 if any((np.frombuffer(img[off:off + size], np.uint16) >= 4096).any() for f, (off, size, _) in enumerate(tab) if f not in dm.RAW) else 0
    else:
        enc = dm.pack(k, img)[0]
    return enc if enc else dec


@pytest.mark.parametrize("k", tc.KS)
def test_status_table_host_codecs_against_the_model(k, api):
    """every (from, to) pair on the cases of tests/transcode_cases.py: the host codecs' statuses, the model's and the ones the cases are
    named for are the same; where both produce a dense record or an image from a dense record, the bytes are the same too"""
    imgs = tc.image_cases(k)
    by_compact = {}
    for name in tc.COMPACT_BATCH:
        rc, rec = tc.compress(api, k, imgs[name])
        assert rc == 0
        by_compact[rec] = imgs[name]
        assert tc.decompress(api, k, rec) == imgs[name]
    seen = set()
    for frm, to in tc.PAIRS:
        for batch in tc.inputs_for(api, k, frm):
            assert len(batch) == 5
            for name, rec in batch:
                want = tc.expected_status(frm, to, name)
                st, out = tc.host_transcode(api, k, frm, to, rec)
                assert st == want, (k, tc.FMT_NAMES[frm], tc.FMT_NAMES[to], name, st, want)
                assert _model_transcode(k, frm, to, rec, by_compact) == want, (k, tc.FMT_NAMES[frm], tc.FMT_NAMES[to], name)
                assert (out is None) == (st < 0)
                if frm == tc.FMT_IMAGE and to == tc.FMT_DENSE and st == 0:
                    assert dm.pack(k, rec) == (0, out)
                if frm == tc.FMT_DENSE and to == tc.FMT_IMAGE:
                    assert dm.unpack(k, rec) == (st, out)
                seen.add((frm, to, want))
    # every status the contract knows occurs: -1 and -2 to dense, -1 to compact, 1 from dense
    for want in ((0, 2, -1), (0, 2, -2), (0, 1, -1), (1, 2, -2), (2, 0, 1), (2, 1, 1)):
        assert want in seen, want


@pytest.mark.parametrize("k", tc.KS)
def test_model_check_on_the_cases(k):
    """model_check (what the check kernel is held to) says 0 / 1 / 2 as the image cases are named"""
    imgs = tc.image_cases(k)
    for name, img in imgs.items():
        want = {0: 0, -1: None, -2: 1 if name == "bad_I" else 2}[tc.IMAGE_STATUS[name][0]]
        if want is not None:
            assert tc.model_check(k, img) == want, (k, name)
    assert tc.model_check(k, imgs["dropped_big"]) == 2 and tc.model_check(k, imgs["other_big"]) == 0
