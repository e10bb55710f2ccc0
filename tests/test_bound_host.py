"""Context-bound proofs (format kosk-bind-v1), the part that needs no GPU: the ABI (header, api.EXPORTS, the built
library), kosk_bind_value and the bound host Fiat-Shamir functions against hashlib restatements, and the CPU model that
tests/bound_oracle.py derives from the oracle: with no binding set it IS the oracle, with one set it accepts exactly its own proofs, and its
proof digests equal tests/golden/bound_v1.json (which pins the format across machines; it does not come from the reference, which has no
such mode).  Every comparison is exact."""
import ctypes as C
import hashlib
import json
import os
import subprocess

import numpy as np
import pytest

from tests import bound_oracle as bo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (2, 3, 4)
NAMES = ["kosk_bind_value", "kosk_bind_device", "kosk_fs_alpha_bound", "kosk_fs_opened_bound", "kosk_fs_alpha_bound_device",
         "kosk_fs_opened_bound_device", "kosk_set_contexts"]
Q, NPARTY, NOPEN = 3329, 1454, 150


def alpha_restated(k, table, bind=b""):
    """alpha_i = BE16(SHAKE256(SHA3-256(table || B) || 01)) % q, 70 + 2K entries"""
    h1 = hashlib.sha3_256(table + bind).digest()
    a = hashlib.shake_256(h1 + b"\x01").digest(2 * (70 + 2 * k))
    return [((a[2 * i] << 8) | a[2 * i + 1]) % Q for i in range(70 + 2 * k)], h1


def opened_restated(table, bind=b""):
    """I: candidates BE16 % 1454 from SHAKE256(SHA3-256(table || B) || 01), each moved to the first free party at or behind it, cyclically"""
    ch = hashlib.sha3_256(table + bind).digest()
    s = hashlib.shake_256(ch + b"\x01").digest(2 * NOPEN)
    used, I = set(), []
    for i in range(NOPEN):
        v = ((s[2 * i] << 8) | s[2 * i + 1]) % NPARTY
        while v in used:
            v = (v + 1) % NPARTY
        used.add(v)
        I.append(v)
    return I, [p for p in range(NPARTY) if p not in used], ch


def random_table(seed):
    return hashlib.shake_256(b"kosk-bind-test-table:%d" % seed).digest(NPARTY * 32)


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "bound_v1.json")) as f:
        return json.load(f)


def test_abi_names():
    from mpcith_kyber_kosk_amd import api
    hdr = open(os.path.join(ROOT, "include", "kosk_mi355x.h")).read()
    for name in NAMES:
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib, name), name
    for name in ("set_contexts", "clear_contexts", "bind_device", "fs_alpha_bound_device", "fs_opened_bound_device"):
        assert callable(getattr(api.Kosk, name)), name
    assert callable(api.bind_value)
    compat = open(os.path.join(ROOT, "include", "kosk_compat.hpp")).read()
    assert "kyber_verifiable_keygen_bound" in compat and "kyber_kosk_verify_bound" in compat


@pytest.mark.parametrize("k", KS)
def test_bind_value_is_the_hashlib_restatement(k, golden):
    from mpcith_kyber_kosk_amd import api
    from tests.golden.make_bound_vectors import bind_cases
    seen = 0
    for kk, pk, ctx in bind_cases():
        if kk != k:
            continue
        want = bo.bind_value(k, pk, ctx)
        assert api.bind_value(k, pk, ctx) == want
        rec = [r for r in golden["bind"] if r["K"] == k and r["context"] == ctx.hex()]
        assert len(rec) == 1 and rec[0]["B"] == want.hex() and rec[0]["pk_sha3_256"] == hashlib.sha3_256(pk).hexdigest()
        seen += 1
    assert seen == 3
    out = C.create_string_buffer(32)
    assert api.lib.kosk_bind_value(5, C.c_char_p(bytes(800)), C.c_char_p(bytes(32)), out) == -1
    assert api.lib.kosk_bind_value(k, None, C.c_char_p(bytes(32)), out) == -1


@pytest.mark.parametrize("k", KS)
def test_bound_host_challenges_against_hashlib(k):
    from mpcith_kyber_kosk_amd import api
    for seed in range(3):
        table = random_table(10 * k + seed)
        bind = hashlib.sha3_256(b"kosk-bind-test-B:%d:%d" % (k, seed)).digest()
        alpha = np.zeros(70 + 2 * k, np.uint16)
        assert api.lib.kosk_fs_alpha_bound(k, C.c_char_p(table), C.c_char_p(bind), alpha.ctypes.data) == 0
        assert alpha.tolist() == alpha_restated(k, table, bind)[0]
        I, rest = np.zeros(NOPEN, np.uint16), np.zeros(NPARTY - NOPEN, np.uint16)
        assert api.lib.kosk_fs_opened_bound(C.c_char_p(table), C.c_char_p(bind), I.ctypes.data, rest.ctypes.data) == 0
        wI, wrest, _ = opened_restated(table, bind)
        assert I.tolist() == wI and rest.tolist() == wrest
        # the unbound functions on the same table still give the unbound values
        assert api.lib.kosk_fs_alpha(k, C.c_char_p(table), alpha.ctypes.data) == 0
        assert alpha.tolist() == alpha_restated(k, table)[0] != alpha_restated(k, table, bind)[0]
        assert api.lib.kosk_fs_opened(C.c_char_p(table), I.ctypes.data, rest.ctypes.data) == 0
        assert I.tolist() == opened_restated(table)[0]


def test_substitution_sites_are_exactly_two():
    src = bo.derived_source()
    assert src.count("ko_bound_sha3(h1, tcomm_all") == 1 and src.count("ko_bound_sha3(ch, digests_all") == 1
    for site in bo.SITES:
        assert site not in src


@pytest.mark.parametrize("k", KS)
def test_model_without_binding_is_the_oracle(k, oracle):
    tape = oracle.tape_bytes_for(k, 0)
    opk, osk, opi, _, _ = oracle.verifiable_keygen(k, tape)
    assert bo.verifiable_keygen(k, tape) == (opk, osk, opi)
    assert bo.verify(k, opi, opk)


@pytest.mark.parametrize("k", KS)
def test_model_with_binding(k, oracle, golden):
    pk, sk, pi = bo.pinned(k)
    opk, osk, opi, _, _ = oracle.verifiable_keygen(k, oracle.tape_bytes_for(k, 0))
    assert (pk, sk) == (opk, osk) and pi != opi and len(pi) == len(opi)  # the same key, another transcript, the same image size
    assert bo.verify(k, pi, pk, context=bo.PIN_CONTEXT)
    B = bo.bind_value(k, pk, bo.PIN_CONTEXT)
    for other in (bytes([B[0] ^ 1]) + B[1:], B[:31] + bytes([B[31] ^ 0x80]), bytes(32),
                  bo.bind_value(k, pk, bytes([bo.PIN_CONTEXT[0] ^ 1]) + bo.PIN_CONTEXT[1:])):
        assert not bo.verify(k, pi, pk, bind=other)
    assert not bo.verify(k, opi, opk, context=bo.PIN_CONTEXT)  # the unbound proof under a binding
    assert not bo.verify(k, pi, pk)                           # the bound proof with no binding set ...
    assert oracle.kosk_verify(k, pi, pk)[0] is False          # ... and at the plain oracle
    rec = golden["proofs"][str(k)]
    assert rec["B"] == B.hex() and rec["pk_sha3_256"] == hashlib.sha3_256(pk).hexdigest()
    assert rec["proof_sha3_256"] == hashlib.sha3_256(pi).hexdigest()


def test_batch_forms_with_suffix_at_every_simd_width(tmp_path):
    """tools/bound_host_check.cpp, a stand-alone program built with ASan + UBSan from csrc/kosk_host.cpp: the multi-buffer hash's suffix
    argument (AVX-512 x 8, AVX2 / AVX-512VL x 4, scalar) against the plain sponge on `table || B`; widths the CPU lacks fall back to the
    next one, which the program reports"""
    exe = str(tmp_path / "bound_host_check")
    r = subprocess.run(["c++", "-std=c++20", "-O1", "-g", "-w", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                        "-I", os.path.join(ROOT, "mpcith_kyber_kosk_amd", "csrc"), os.path.join(ROOT, "tools", "bound_host_check.cpp"),
                        os.path.join(ROOT, "mpcith_kyber_kosk_amd", "csrc", "kosk_host.cpp"), "-lpthread", "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    for extra in ({}, {"KOSK_FS_WIDTH": "4"}, {"KOSK_FS_WIDTH": "1"}, {"KOSK_HOST_SCALAR": "1"}):
        env = dict(os.environ, **extra)
        r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
        assert r.returncode == 0 and "mismatches 0" in r.stdout, (extra, r.stdout[-3000:])
