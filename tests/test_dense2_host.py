"""Host side of the dense wire format kosk-dense-v2, no GPU: the names, the sizes, the host codec
(kosk_dense2_proof_bytes, kosk_proof_dense2_pack, kosk_proof_dense2_unpack) against the numpy model tests/dense2_model.py and the pinned
values of tests/golden/dense_v2.json, every return code, and the host status table of all 12 transcoding pairs as the composition of the
codecs."""
import ctypes as C
import hashlib
import json
import os
import re

import numpy as np
import pytest

from tests import dense2_cases as dc
from tests import dense2_model as d2
from tests import dense_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (2, 3, 4)
SIZES = {2: 247552, 3: 252512, 4: 269600}
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "dense_v2.json")))
NAMES = ["kosk_dense2_proof_bytes", "kosk_proof_dense2_pack", "kosk_proof_dense2_unpack", "kosk_dense2_fill_device", "kosk_dense2_check_device",
         "kosk_verifiable_keygen_batch_fmt", "kosk_verifiable_keygen_seeded_batch_fmt", "kosk_verify_batch_fmt", "kosk_fetch_proofs_fmt",
         "kosk_stage_verifier_inputs_fmt"]


@pytest.fixture(scope="module")
def api():
    from mpcith_kyber_kosk_amd import api
    return api


oracle_proof, _u16, _set_u16, _at = dc.oracle_proof, dc.get16, dc.put16, dc.at


def test_names_are_declared_bound_and_exported(api):
    header = open(os.path.join(ROOT, "include", "kosk_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in api.EXPORTS and hasattr(api.lib, name) and getattr(api.lib, name).argtypes is not None, name
    for name in NAMES[5:]:
        assert re.search(r"\bint %s\s*\(kosk_ctx \*ctx, int fmt," % name, code), name      # fmt right behind ctx
    assert re.search(r"enum\s*\{\s*KOSK_FMT_DENSE2 = 4\s*\}", code)
    assert re.search(r"enum\s*\{\s*KOSK_FMT_IMAGE = 0,\s*KOSK_FMT_COMPACT = 1,\s*KOSK_FMT_DENSE = 2\s*\}", code)
    assert re.search(r"3 is not a format", header)
    assert api.FMT_DENSE2 == 4 and (api.FMT_IMAGE, api.FMT_COMPACT, api.FMT_DENSE) == (0, 1, 2)
    assert api.Kosk.PATH_DENSE2_FILL == 23 and api.Kosk.PATH_DENSE2_CHECK == 24
    assert api.Kosk._FMT[api.FMT_DENSE2][1] == "kosk_dense2_proof_bytes"
    for method in ("verifiable_keygen_dense2", "verify_dense2", "fetch_proofs_dense2", "stage_verifier_inputs_dense2", "dense2_fill_device",
                   "dense2_check_device"):
        assert callable(getattr(api.Kosk, method)), method
    for fn in ("format_bytes", "proof_dense2_pack", "proof_dense2_unpack"):
        assert callable(getattr(api, fn)), fn


@pytest.mark.parametrize("k", KS)
def test_sizes_from_library_model_and_fixture(k, api):
    g = GOLDEN["k"][str(k)]
    assert d2.dense2_bytes(k) == SIZES[k] == g["dense2_bytes"]
    assert api.lib.kosk_dense2_proof_bytes(k) == SIZES[k] == api.lib.kosk_format_bytes(k, 4) == api.format_bytes(k, api.FMT_DENSE2)
    assert d2.image_bytes(k) == g["image_bytes"] == api.proof_bytes(k)
    assert api.lib.kosk_format_bytes(k, 3) == 0 and api.lib.kosk_format_bytes(k, 5) == 0
    assert api.lib.kosk_format_bytes(k, 2) == dm.dense_bytes(k) > SIZES[k]              # v1 as it was
    assert api.lib.kosk_dense2_proof_bytes(1) == 0 and api.lib.kosk_dense2_proof_bytes(5) == 0 and api.lib.kosk_format_bytes(5, 4) == 0


@pytest.mark.parametrize("k", KS)
def test_pack_equals_the_model_and_round_trips(k, api):
    pi = oracle_proof(k)
    rc, rec = api.proof_dense2_pack(k, pi)
    assert rc == 0
    assert (0, rec) == d2.pack(k, pi), "host pack differs from the model"
    assert hashlib.sha256(rec).hexdigest() == GOLDEN["k"][str(k)]["record_sha256"]
    assert api.proof_dense2_unpack(k, rec) == (0, pi), "unpack(pack(pi)) != pi"
    assert d2.unpack(k, rec) == (0, pi)
    # an old record is what it was
    assert api.dense_pack(k, pi) == dm.pack(k, pi)


@pytest.mark.parametrize("k", KS)
def test_return_codes_of_pack(k, api):
    pi = oracle_proof(k)
    tab, _ = d2.field_table(k)

    def both(img):
        rc = api.proof_dense2_pack(k, bytes(img))[0]
        assert rc == d2.pack(k, bytes(img))[0], "library and model disagree"
        return rc
    for f in (15, 16, 21, 22):
        R = d2.ROWS[f]
        # -1: a stored 4096 at row 0 and at row R - 1
        for row, col in ((0, 0), (R - 1, -1)):
            img = bytearray(pi); _set_u16(img, _at(k, f, row, col), 4096)
            assert both(img) == -1, (k, f, row)
        # -2: a 4096 in a dropped row; -1 wins when both are present
        img = bytearray(pi); _set_u16(img, _at(k, f, R, 0), 4096)
        assert both(img) == -2, (k, f)
        _set_u16(img, _at(k, f, 3, 1), 4096)
        assert both(img) == -1, (k, f)
        # -2: v + q in a dropped row (congruent, not canonical)
        at = _at(k, f, R + 5, 0)
        while _u16(pi, at) + d2.Q >= 4096:
            at += 2
        img = bytearray(pi); _set_u16(img, at, _u16(pi, at) + d2.Q)
        assert both(img) == -2, (k, f)
        # -2: one changed u16 at rows R - 1, R and 1303
        for row, col in ((R - 1, 0), (R, -1), (d2.NREST - 1, -1)):
            img = bytearray(pi)
            at = _at(k, f, row, col)
            _set_u16(img, at, (_u16(img, at) + 1) % d2.Q)
            assert both(img) == -2, (k, f, row)
    # "+1 on a whole eta column": still degree <= 406, other secrets -> v1 packs it, v2 does not
    off, size, cols = tab[15]
    v = np.frombuffer(pi[off:off + size], np.uint16).reshape(d2.NREST, cols).astype(np.int64)
    v[:, 2] = (v[:, 2] + 1) % d2.Q
    img = pi[:off] + v.astype(np.uint16).tobytes() + pi[off + size:]
    assert api.dense_pack(k, img)[0] == 0 and dm.pack(k, img)[0] == 0
    assert both(img) == -2
    # a nonzero constant on a whole u column is no codeword either
    off, size, cols = tab[21]
    v = np.frombuffer(pi[off:off + size], np.uint16).reshape(d2.NREST, cols).astype(np.int64)
    v[:, 0] = (v[:, 0] + 7) % d2.Q
    assert both(pi[:off] + v.astype(np.uint16).tobytes() + pi[off + size:]) == -2
    # malformed I
    oi = tab[d2.F_I][0]
    img = bytearray(pi); _set_u16(img, oi + 2, _u16(img, oi))
    assert both(img) == -2
    img = bytearray(pi); _set_u16(img, oi + 2 * 149, d2.NPARTY)
    assert both(img) == -2
    # NULL and bad K
    out = C.create_string_buffer(SIZES[k])
    img = C.create_string_buffer(len(pi))
    assert api.lib.kosk_proof_dense2_pack(5, pi, out) == -1 and api.lib.kosk_proof_dense2_pack(k, None, out) == -1
    assert api.lib.kosk_proof_dense2_pack(k, pi, None) == -1
    assert api.lib.kosk_proof_dense2_unpack(1, out, img) == -1 and api.lib.kosk_proof_dense2_unpack(k, None, img) == -1
    assert api.lib.kosk_proof_dense2_unpack(k, out, None) == -1


@pytest.mark.parametrize("k", KS)
def test_values_between_q_and_4095_survive_raw(k, api):
    """kept values in [q, 4095]: stored and returned as they are, folded mod q for the refill; the refilled rows are canonical"""
    pi = oracle_proof(k)
    tab, _ = d2.field_table(k)
    img = bytearray(pi)
    for f, row, col, v in ((15, 0, 0, 4095), (16, 150, -1, d2.Q), (21, 556, -1, 3500), (22, 7, 1, 4000), (2, 3, 1, 4095)):
        _set_u16(img, _at(k, f, row, col), v)
    assert d2.refill(k, img) == 0                       # the codeword of these kept rows
    img = bytes(img)
    assert img != pi
    rc, rec = api.proof_dense2_pack(k, img)
    assert rc == 0 and (0, rec) == d2.pack(k, img)
    assert api.proof_dense2_unpack(k, rec) == (0, img)
    for f in d2.LISTED:
        off, size, cols = tab[f]
        assert (np.frombuffer(img[off + d2.ROWS[f] * cols * 2:off + size], np.uint16) < d2.Q).all()


@pytest.mark.parametrize("k", KS)
def test_unpack_of_a_malformed_opened_list(k, api):
    """unpack result 1, and exactly the stated rows are zero: 407.. of the five v1 fields, 151.. of fields 15 / 16, 557.. of fields 21 / 22"""
    pi = oracle_proof(k)
    tab, _ = d2.field_table(k)
    lay, _ = d2.record_layout(k)
    rec = bytearray(api.proof_dense2_pack(k, pi)[1])
    ro, rb = lay[d2.F_I]
    opened = d2.unpack12(bytes(rec[ro:ro + rb]), d2.NOPEN)
    for pos, val in ((7, int(opened[3])), (0, d2.NPARTY), (149, 4095)):
        bad = opened.copy(); bad[pos] = val
        r2 = bytearray(rec); r2[ro:ro + rb] = d2.pack12(bad).tobytes()
        st, img = api.proof_dense2_unpack(k, bytes(r2))
        assert st == 1 and (st, img) == d2.unpack(k, bytes(r2))
        want = bytearray(pi)
        want[tab[d2.F_I][0]:tab[d2.F_I][0] + 2 * d2.NOPEN] = bad.tobytes()
        for f, R in (list((f, 407) for f in (2, 3, 8, 13, 14)) + [(15, 151), (16, 151), (21, 557), (22, 557)]):
            off, size, cols = tab[f]
            want[off + R * cols * 2:off + size] = bytes(size - R * cols * 2)
        assert img == bytes(want)


# ---- the status table of kosk_transcode_batch for all 12 ordered pairs, as the composition of the host codecs (tests/dense2_cases.py)
@pytest.mark.parametrize("k", KS)
def test_status_table_of_all_twelve_pairs(k, api):
    cases = dc.transcode_images(k)
    pairs = dc.PAIRS
    host_transcode = dc.host_transcode
    assert len(pairs) == 12
    col = {1: 1, 2: 2, 4: 3}
    seen = set()
    for name, row in cases.items():
        img = row[0]
        for to in (1, 2, 4):
            st, rec = host_transcode(api, k, 0, to, img)
            assert st == row[col[to]], (k, name, to, st)
            seen.add((0, to, st))
            if st < 0:
                continue
            # a record that exists: back to the image and on into the two other packed formats
            assert host_transcode(api, k, to, 0, rec) == (0, img), (k, name, to)
            seen.add((to, 0, 0))
            for to2 in (1, 2, 4):
                if to2 != to:
                    st2, rec2 = host_transcode(api, k, to, to2, rec)
                    assert st2 == row[col[to2]], (k, name, to, to2, st2)
                    if st2 == 0:
                        assert rec2 == host_transcode(api, k, 0, to2, img)[1]
                    seen.add((to, to2, st2))
    # records with a malformed I: decoder status 1 towards the image and compact, -2 towards the other dense format
    for fmt, layout, other in ((4, d2.record_layout(k)[0], 2), (2, dm.record_layout(k)[0], 4)):
        rec = dc.bad_I_record(k, host_transcode(api, k, 0, fmt, cases["ok"][0])[1], layout, "dup")
        assert host_transcode(api, k, fmt, 0, rec)[0] == 1 and host_transcode(api, k, fmt, 1, rec)[0] == 1
        assert host_transcode(api, k, fmt, other, rec) == (-2, None)
        seen.update({(fmt, 0, 1), (fmt, 1, 1), (fmt, other, -2)})
    for pair in pairs:
        assert (pair[0], pair[1], 0) in seen, pair
    for want in ((0, 4, -1), (0, 4, -2), (1, 4, -2), (2, 4, -2), (4, 0, 1), (4, 1, 1), (4, 2, -2), (2, 4, 0), (4, 2, 0)):
        assert want in seen, want
