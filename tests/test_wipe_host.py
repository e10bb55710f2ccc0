"""Erasing secrets, the parts that need no GPU: the five names are declared, bound and exported, their NULL-argument
returns, the header's path-id list, and the needles of the GPU tests (tests/wipe_cases.py) that can be computed on the host."""
import ctypes as C
import os
import re

import pytest

from tests import wipe_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kosk_wipe_secrets", "kosk_set_wipe", "kosk_secret_scan", "kosk_wipe_device", "kosk_wipe_timing"]


@pytest.fixture(scope="module")
def api():
    from mpcith_kyber_kosk_amd import api
    return api


def _header():
    return open(os.path.join(ROOT, "include", "kosk_mi355x.h")).read()


def test_names_are_declared_bound_and_exported(api):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(kosk_ctx \*ctx" % name, code), name
        assert name in api.EXPORTS and hasattr(api.lib, name), name
        assert getattr(api.lib, name).argtypes is not None, name
    assert re.search(r"enum\s*\{\s*KOSK_WIPE_OFF = 0,\s*KOSK_WIPE_CALL = 1\s*\}", code)
    assert (api.WIPE_OFF, api.WIPE_CALL) == (0, 1) and api.Kosk.PATH_WIPE == 18
    for method in ("wipe_secrets", "set_wipe", "secret_scan", "wipe_device"):
        assert callable(getattr(api.Kosk, method))


def test_null_arguments_return_minus_one(api):
    lib = api.lib
    assert lib.kosk_wipe_secrets(None) == -1
    assert lib.kosk_set_wipe(None, 1) == -1
    hits = C.c_long(7)
    assert lib.kosk_secret_scan(None, C.c_char_p(bytes(range(32))), 32, C.byref(hits)) == -1 and hits.value == 7
    assert lib.kosk_wipe_device(None, 0, None, None) == -1
    assert lib.kosk_wipe_timing(None, 1, None, None, None, None) == -1


def test_header_lists_path_id_18():
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int kosk_path_count\(", _header(), flags=re.S)
    assert m and re.search(r"\b18 launches of k_wipe\b", m.group(1)) and re.search(r"\b17 launches of k_keyseed\b", m.group(1))


def test_caveats_point_to_section_13():
    """no "until a later call overwrites it or the handle is destroyed" is left standing as an open caveat"""
    for path in ("include/kosk_mi355x.h", "INTEGRATION.md"):
        text = " ".join(open(os.path.join(ROOT, path)).read().split())
        for m in re.finditer(r"overwrites (?:it|them) or the handle is destroyed", text):
            assert re.search(r"(?:INTEGRATION\.md 13|§13)", text[m.start():m.start() + 400]), (path, text[m.start() - 80:m.start() + 120])
    assert re.search(r"^## 13\.", open(os.path.join(ROOT, "INTEGRATION.md")).read(), flags=re.M)


@pytest.mark.parametrize("k", wc.KS)
def test_no_needle_is_a_run_of_one_byte_value(k, api):
    """Needle() asserts it for every needle the GPU tests make; here for the ones the host can compute: tape and seed bytes, the derived
    seed, z and the packed NTT(s) of an sk, coins, and both forms of the first 32 coefficients of s"""
    t = wc.tape(k, 0)
    needles = wc.tape_needles(t) + wc.s_needles(k, t[:64]) + [wc.Needle("seed", wc.seed(0)), wc.Needle("m", wc.coins32(0)),
                                                              wc.Needle("d", wc.coins64(0)[:32]), wc.Needle("z", wc.coins64(0)[32:])]
    pks, sks = wc.honest_keys(k, 1)
    needles += wc.sk_needles(sks[0]) + [wc.Needle("derived seed", api.keyseed_value(k, sks[0])), wc.control(pks[0])]
    assert len({n.data for n in needles}) == len(needles)
    lens = sorted({len(n.data) for n in needles})
    assert lens == [32, 64]
    with pytest.raises(AssertionError):
        wc.Needle("zeros", bytes(32))
    s16, u16 = wc.s_needles(k, t[:64])
    assert s16.data != u16.data  # a negative coefficient among the first 32: the two forms differ
