"""Host tests of the offline bank's interface: the names, the argument checks that need no handle, the tape sections
against the formula, the entry size, the header's path ids.  No GPU."""
import ctypes as C
import os
import re

import pytest

from tests import bank_cases as bc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kosk_bank_entry_bytes", "kosk_tape_section", "kosk_bank_reserve", "kosk_bank_level", "kosk_bank_fill", "kosk_stage_prover_keys_banked",
         "kosk_prove_keys_banked_batch", "kosk_verifiable_keygen_banked_batch"]


def _header():
    with open(os.path.join(ROOT, "include", "kosk_mi355x.h")) as f:
        return f.read()


def test_the_eight_names_are_declared_bound_and_exported():
    from mpcith_kyber_kosk_amd import api
    header = _header()
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in api.EXPORTS, name
        fn = getattr(api.lib, name)
        assert fn.argtypes is not None, name
    for method in ("bank_reserve", "bank_level", "bank_fill", "stage_prover_keys_banked", "prove_keys_banked", "verifiable_keygen_banked"):
        assert callable(getattr(api.Kosk, method)), method


def test_null_and_bad_arguments_without_a_handle():
    from mpcith_kyber_kosk_amd import api
    lib = api.lib
    off, size = C.c_size_t(7), C.c_size_t(7)
    for k in (1, 5, 0, -3):
        assert lib.kosk_bank_entry_bytes(k) == 0
        assert lib.kosk_tape_section(k, 0, C.byref(off), C.byref(size)) == -1
    for section in (-1, 3, 99):
        assert lib.kosk_tape_section(3, section, C.byref(off), C.byref(size)) == -1
    assert (off.value, size.value) == (7, 7)  # a refused call writes nothing
    assert lib.kosk_tape_section(3, 1, None, C.byref(size)) == -1
    assert lib.kosk_tape_section(3, 1, C.byref(off), None) == -1
    buf = C.create_string_buffer(64)
    r, c = C.c_int(), C.c_int()
    assert lib.kosk_bank_reserve(None, 4) == -1
    assert lib.kosk_bank_level(None, C.byref(r), C.byref(c)) == -1
    assert lib.kosk_bank_fill(None, 1, None, 0, None, 0) == -1
    assert lib.kosk_stage_prover_keys_banked(None, 1, buf, None, 0, None, 0, buf) == -1
    assert lib.kosk_prove_keys_banked_batch(None, 1, buf, None, 0, None, 0, buf, buf) == -1
    assert lib.kosk_verifiable_keygen_banked_batch(None, 1, None, 0, None, 0, buf, buf, buf) == -1


@pytest.mark.parametrize("k", bc.KS)
def test_tape_sections_follow_the_formula_and_tile_the_tape(k):
    from mpcith_kyber_kosk_amd import api
    M, E, eta1, T, O = bc.shape(k)
    assert T == api.tape_bytes(k)
    got = [api.tape_section(k, s) for s in range(3)]
    assert got == [(0, 64), (64, O - 64), (O, T - O)] == bc.sections(k)
    assert O - 64 == 32 * M + 302 * (2 * M + 2 * k * E)
    assert T - O == 302 * (3 * k + 4 * k * eta1)
    end = 0
    for off, size in got:
        assert off == end and size > 0
        end = off + size
    assert end == T
    # the python splice helper agrees with the sections
    a, b = bc.tape(k, 0, "a"), bc.tape(k, 0, "b")
    sp = api.tape_splice(k, a, b)
    assert sp == bc.splice(k, a, b) and len(sp) == T
    assert sp[:64] == b[:64] and sp[64:O] == a[64:O] and sp[O:] == b[O:]


@pytest.mark.parametrize("k", bc.KS)
def test_entry_bytes_hold_the_offline_rows(k):
    from mpcith_kyber_kosk_amd import api
    M, E, _eta1, _T, _O = bc.shape(k)
    need = (2 * M + 2 * k * E) * bc.RS_COLUMNS * 2
    got = api.bank_entry_bytes(k)
    assert got >= need and got % 16 == 0, (got, need)


def test_the_header_lists_the_path_ids():
    from mpcith_kyber_kosk_amd import api
    header = _header()
    m = re.search(r"/\* Which kernel / copy paths ran.*?\*/\s*int kosk_path_count", header, re.S)
    assert m
    text = m.group(0)
    assert re.search(r"\b25 launches of k_bank_put\b", text) and re.search(r"\b26 launches of k_bank_take\b", text)
    assert api.Kosk.PATH_BANK_PUT == 25 and api.Kosk.PATH_BANK_TAKE == 26
