"""Host codec of the dense wire format kosk-dense-v1 (kosk_dense_proof_bytes, kosk_proof_dense_pack, kosk_proof_dense_unpack) against
the numpy model of the format (tests/dense_model.py) and the pinned sizes and digests of tests/golden/dense_v1.json.  No GPU."""
import functools
import hashlib
import json
import os

import numpy as np
import pytest

from tests import dense_model as dm

KS = (2, 3, 4)
GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dense_v1.json")))


@pytest.fixture(scope="module")
def api():
    from mpcith_kyber_kosk_amd import api
    return api


@functools.lru_cache(maxsize=None)
def oracle_proof(k):
    from tests import oracle_lib
    return oracle_lib.verifiable_keygen(k, oracle_lib.tape_bytes_for(k, 0))[2]


def _u16(img, off):
    return img[off] | (img[off + 1] << 8)


def _set_u16(img, off, v):
    img[off] = v & 0xFF
    img[off + 1] = v >> 8


@pytest.mark.parametrize("k", KS)
def test_sizes_match_the_golden_values(k, api):
    g = GOLDEN["k"][str(k)]
    assert dm.dense_bytes(k) == g["dense_bytes"] and dm.image_bytes(k) == g["image_bytes"] == api.proof_bytes(k)
    assert api.dense_proof_bytes(k) == g["dense_bytes"]
    assert g["dense_bytes"] % 16 == 0 and 0.42 < g["dense_bytes"] / g["image_bytes"] < 0.44
    assert api.dense_proof_bytes(1) == 0 and api.dense_proof_bytes(5) == 0


@pytest.mark.parametrize("k", KS)
def test_pack_equals_the_model_and_round_trips(k, api):
    pi = oracle_proof(k)
    rc, rec = api.dense_pack(k, pi)
    assert rc == 0
    assert (0, rec) == dm.pack(k, pi), "host pack differs from the model"
    assert hashlib.sha3_256(rec).hexdigest() == GOLDEN["k"][str(k)]["record_sha3_256"]
    assert api.dense_unpack(k, rec) == (0, pi), "unpack(pack(pi)) != pi"
    assert dm.unpack(k, rec) == (0, pi)


@pytest.mark.parametrize("k", KS)
def test_changed_dropped_rows_are_refused(k, api):
    """one u16 in row 407, in row 1303 and in a middle row of each of the seven fields: -2"""
    pi = oracle_proof(k)
    tab, _ = dm.field_table(k)
    for f in dm.LISTED:
        off, size, cols = tab[f]
        for row, col in ((dm.KEPT, 0), (dm.NREST - 1, cols - 1), (850, cols // 2)):
            img = bytearray(pi)
            at = off + (row * cols + col) * 2
            _set_u16(img, at, (_u16(img, at) + 1) % dm.Q)
            assert api.dense_pack(k, bytes(img))[0] == -2, (k, f, row, col)
            assert dm.pack(k, bytes(img))[0] == -2
    # the same change in a kept row gives another codeword's kept row, not this image's dropped rows: -2 as well
    img = bytearray(pi)
    at = tab[2][0] + 10
    _set_u16(img, at, (_u16(img, at) + 1) % dm.Q)
    assert api.dense_pack(k, bytes(img))[0] == -2


@pytest.mark.parametrize("k", KS)
def test_return_codes(k, api):
    pi = oracle_proof(k)
    tab, _ = dm.field_table(k)
    # -1: a value >= 4096 in a kept row of a truncated field, and in a field that is stored whole
    for f, idx in ((2, 406 * dm.NCHK + 69), (8, 0), (0, 17), (21, 5)):
        img = bytearray(pi)
        _set_u16(img, tab[f][0] + 2 * idx, 4096)
        assert api.dense_pack(k, bytes(img))[0] == -1, (k, f)
        assert dm.pack(k, bytes(img))[0] == -1
    # -2: duplicated and out-of-range opened parties
    oi = tab[dm.F_I][0]
    img = bytearray(pi); _set_u16(img, oi + 2, _u16(img, oi))
    assert api.dense_pack(k, bytes(img))[0] == -2 and dm.pack(k, bytes(img))[0] == -2
    img = bytearray(pi); _set_u16(img, oi + 2 * 149, dm.NPARTY)
    assert api.dense_pack(k, bytes(img))[0] == -2 and dm.pack(k, bytes(img))[0] == -2
    # a changed value in field 21 (degree 812: stored whole) still packs, and comes back
    img = bytearray(pi)
    at = tab[21][0] + 2 * 1000
    _set_u16(img, at, (_u16(img, at) + 1) % dm.Q)
    rc, rec = api.dense_pack(k, bytes(img))
    assert rc == 0 and (0, rec) == dm.pack(k, bytes(img)) and api.dense_unpack(k, rec) == (0, bytes(img))
    # bad arguments
    assert api.lib.kosk_proof_dense_pack(5, pi, rec) == -1 and api.lib.kosk_proof_dense_unpack(k, None, rec) == -1


@pytest.mark.parametrize("k", KS)
def test_values_between_q_and_4095_survive_raw(k, api):
    """kept values in [q, 4095]: stored and returned as they are, folded mod q for the refill; the refilled rows are the model's"""
    pi = oracle_proof(k)
    tab, _ = dm.field_table(k)
    img = bytearray(pi)
    for f, idx, v in ((2, 3 * dm.NCHK + 1, 4095), (3, 0, dm.Q), (8, 406 * k, 3500), (16, 77, 4000)):
        _set_u16(img, tab[f][0] + 2 * idx, v)
    assert dm.refill(k, img) == 0                       # the codeword of these kept rows
    img = bytes(img)
    assert img != pi
    rc, rec = api.dense_pack(k, img)
    assert rc == 0 and (0, rec) == dm.pack(k, img)
    st, back = api.dense_unpack(k, rec)
    assert st == 0 and back == img
    for f in dm.LISTED:                                 # refilled rows are canonical
        off, size, cols = tab[f]
        assert (np.frombuffer(back[off + dm.KEPT * cols * 2:off + size], np.uint16) < dm.Q).all()


@pytest.mark.parametrize("k", KS)
def test_unpack_of_a_malformed_opened_list(k, api):
    pi = oracle_proof(k)
    tab, _ = dm.field_table(k)
    lay, _ = dm.record_layout(k)
    rec = bytearray(api.dense_pack(k, pi)[1])
    ro, rb = lay[dm.F_I]
    opened = dm.unpack12(bytes(rec[ro:ro + rb]), dm.NOPEN)
    for pos, val in ((7, int(opened[3])), (0, dm.NPARTY), (149, 4095)):
        bad = opened.copy(); bad[pos] = val
        r2 = bytearray(rec); r2[ro:ro + rb] = dm.pack12(bad).tobytes()
        st, img = api.dense_unpack(k, bytes(r2))
        assert st == 1 and (st, img) == dm.unpack(k, bytes(r2))
        for f in dm.LISTED:
            off, size, cols = tab[f]
            assert not any(img[off + dm.KEPT * cols * 2:off + size]) and img[off:off + dm.KEPT * cols * 2] == pi[off:off + dm.KEPT * cols * 2]
