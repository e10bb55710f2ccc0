"""The relying party, the parts that need no GPU: the three names are declared with their exact prototype lines, bound
and exported, the three path ids and the header's sentences for them, the refusals that need no handle, the example under -fsyntax-only,
and the crafted-case tables of tests/relying_cases.py, each held against the host function, the hashlib model and what it was crafted
for, so that no GPU case depends on an expectation the reference side does not itself produce."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from tests import registry_sorted_model as sm
from tests import relying_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kosk_regtree_check_paths", "kosk_regsort_check_proofs", "kosk_kem_enc_proven"]
METHODS = ["regtree_check_paths", "regsort_check_proofs", "kem_enc_proven"]
PROTOTYPES = (
    "int kosk_regtree_check_paths(kosk_ctx *ctx, int n, int depth, const int32_t *slots, const uint8_t *state, const uint8_t *h, const uint8_t *paths, const uint8_t root[32], uint8_t *ok);",
    "int kosk_regsort_check_proofs(kosk_ctx *ctx, int n, int depth, const uint8_t *x, const uint8_t *records, const uint8_t root[32], uint8_t *verdict);",
    "int kosk_kem_enc_proven(kosk_ctx *ctx, int n, int depth, const uint8_t *pk, const int32_t *slots, const uint8_t *paths, const uint8_t root[32], const uint8_t *coins, uint8_t *ct, uint8_t *ss, uint8_t *done);",
)
KS = (2, 3, 4)


@pytest.fixture(scope="module")
def api():
    from mpcith_kyber_kosk_amd import api
    return api


def _header():
    return open(os.path.join(ROOT, "include", "kosk_mi355x.h")).read()


def test_names_are_declared_bound_and_exported(api):
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, code), name
        assert name in api.EXPORTS and hasattr(api.lib, name), name
        assert getattr(api.lib, name).argtypes is not None, name
    for method in METHODS:
        assert callable(getattr(api.Kosk, method)), method
    for line in PROTOTYPES:
        assert line + "\n" in code, line
    assert "The relying party (INTEGRATION.md 8.9 is the normative text)" in _header()
    assert _header().index("int kosk_monitor_read(") < _header().index("The relying party (INTEGRATION.md 8.9")


def test_path_ids_and_the_header_sentences(api):
    K = api.Kosk
    assert (K.PATH_REGTREE_CHECK, K.PATH_REGSORT_CHECK, K.PATH_KEM_ENC_PROVEN) == (46, 47, 48)
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int kosk_path_count\(", _header(), flags=re.S)
    assert m
    text = re.sub(r"\s*\n \* ", " ", m.group(1))
    assert "46 launches of k_regtree_check (one per launch group of kosk_regtree_check_paths, and one per launch group of kosk_kem_enc_proven)" in text
    assert "47 launches of k_regsort_check (one per launch group of kosk_regsort_check_proofs)" in text
    assert "48 kem_enc_proven: encapsulation launches of kosk_kem_enc_proven" in text
    # the earlier sentences are still there, word for word
    assert "12 kem_enc / 13 kem_dec: launch groups (up to 16384 items, three or four launches each) of the KEM calls" in text
    assert "31 kem_enc_peers: launch groups of kosk_kem_enc_peers (ids 12 / 20 / 28 do not move for it)" in text
    assert "34 launches of k_registry_path (one per launch group of kosk_registry_prove_slots / kosk_registry_prove_peers)" in text
    assert "37 launches of k_regsort_prove (one per launch group of kosk_registry_prove_absent)" in text
    assert "41 launches of k_reghist_prove (one per launch group of kosk_registry_history_prove_events / _prove_consistency" in text
    assert "42 launches of k_monitor_keys (one per segment of kosk_monitor_feed)" in text
    assert "45 launches of k_monitor_check (one per checkpoint event fed)" in text
    assert "(32, 33, 35, 36, 38..40) on the monitor's handle" in text
    assert "ids 42..45 do not move for kosk_monitor_head, _roots, _read or _level" in text


def test_refusals_without_a_handle(api):
    lib = api.lib
    buf = C.create_string_buffer(4096)
    slots = (C.c_int32 * 1)(0)
    assert lib.kosk_regtree_check_paths(None, 1, 0, slots, None, buf, None, buf, buf) == -1
    assert lib.kosk_regsort_check_proofs(None, 1, 0, buf, buf, buf, buf) == -1
    assert lib.kosk_kem_enc_proven(None, 1, 0, buf, slots, None, buf, buf, buf, buf, buf) == -1
    for n, depth in ((0, 0), (-1, 0), (1, -1), (1, 32)):
        assert lib.kosk_regtree_check_paths(None, n, depth, slots, None, buf, buf, buf, buf) == -1
        assert lib.kosk_regsort_check_proofs(None, n, depth, buf, buf, buf, buf) == -1
        assert lib.kosk_kem_enc_proven(None, n, depth, buf, slots, buf, buf, buf, buf, buf, buf) == -1
    assert buf.raw == bytes(4096)


def test_the_example_parses():
    """examples/registry_relying.cpp against the header, host side only"""
    cxx = shutil.which("hipcc") or shutil.which("c++") or shutil.which("g++")
    assert cxx, "no C++ compiler"
    cmd = [cxx, "-std=c++17", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "registry_relying.cpp")]
    if os.path.basename(cxx) == "hipcc":
        cmd[1:1] = ["-x", "c++"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout


@pytest.mark.parametrize("k", KS)
def test_path_tables_host_function_against_the_model(k, api):
    seen = set()
    for t in cases.all_path_tables(api, k):
        host, model = cases.host_paths(api, t), cases.model_paths(t)
        for c, a, b in zip(t["cases"], host, model):
            assert a == b == c[5], (k, t["depth"], c[0], a, b)
        seen.add(t["depth"])
    assert seen == {0, 1, 9, 11, 12, 31}
    main = cases.path_table(k)
    names = [c[0] for c in main["cases"]]
    assert sum(n.startswith("key ") for n in names) == 130 and sum(bool(re.match(r"empty \d+$", n)) for n in names) == 10
    assert sum(n.startswith("bit flipped at level") for n in names) == cases.D and sum(n.startswith("slot bit") for n in names) == cases.D
    assert all(w == 0 for w in cases.host_paths(api, cases.path_table_bad_root(k))) and len(cases.path_table_bad_root(k)["cases"]) == 140


@pytest.mark.parametrize("k", KS)
def test_proof_tables_host_function_against_the_model(k, api):
    t = cases.proof_table(k)
    host, model = cases.host_proofs(api, t), cases.model_proofs(t)
    assert host == model
    for c, a in zip(t["cases"], host):
        assert c[3] is None or a == c[3], (k, c[0], a)
    names = [c[0] for c in t["cases"]]
    # every return statement of regsort::check_proof that a record can reach is named (R5 needs a full table: below)
    assert {n[:2] for n in names if re.match(r"R\d ", n)} == {"R1", "R2", "R3", "R4", "R6", "R7", "R8"}
    mutated = [a for c, a in zip(t["cases"], host) if c[0].startswith("mutation")]
    assert len(mutated) == cases.MUTATIONS and set(mutated) == {sm.NEITHER, sm.ABSENT, sm.PRESENT}
    assert sum(n == "PRESENT" for n in names) == 130
    full = cases.proof_table_full(k)
    host, model = cases.host_proofs(api, full), cases.model_proofs(full)
    assert host == model
    for c, a in zip(full["cases"], host):
        assert a == c[3], (k, c[0], a)
    assert any(c[0].startswith("R5") for c in full["cases"])
