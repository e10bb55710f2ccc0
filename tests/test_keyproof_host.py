"""Proofs for existing Kyber keys, the part that needs no GPU: the ABI (header, api.EXPORTS, the built library), the fixture
tests/golden/keyproof_keys_v1.json (re-derived from oracle/_ref where that exists -- KOSK_REQUIRE_REF=1 makes its absence a failure --
and its internal checks everywhere), and the witness recovery itself: csrc/kosk_witness_dev.hpp is host/device code,
tools/witness_host_model.cpp builds it for the host and runs a workgroup as one thread.  Expected values come from api.host_keygen
(the key generation's own s, e) and from the pure-Python model in tests/keyproof_cases.py; every comparison is exact."""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import keyproof_cases as kc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = kc.KS
NAMES = ["kosk_witness_from_sk", "kosk_stage_prover_keys", "kosk_stage_prover_keys_seeded", "kosk_prove_keys_batch", "kosk_prove_keys_seeded_batch"]
SEEDS = 8


def test_abi_names():
    from mpcith_kyber_kosk_amd import api
    hdr = open(os.path.join(ROOT, "include", "kosk_mi355x.h")).read()
    for name in NAMES:
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib, name), name
    for name in ("witness_from_sk", "stage_prover_keys", "prove_keys"):
        assert callable(getattr(api.Kosk, name))
    assert "kyber_kosk_prove_key" in open(os.path.join(ROOT, "include", "kosk_compat.hpp")).read()
    assert api.Kosk.PATH_IDS[-1] == "kem_dec"  # no path id was added


def _build(tmp, name, extra):
    exe = str(tmp / name)
    r = subprocess.run(["c++", "-std=c++20"] + extra + ["-I", os.path.join(ROOT, "mpcith_kyber_kosk_amd", "csrc"),
                        os.path.join(ROOT, "tools", "witness_host_model.cpp"), "-o", exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
    return exe


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("witness_model")


@pytest.fixture(scope="module")
def model(workdir):
    exe = _build(workdir, "witness_host_model", ["-O2"])
    count = [0]

    def run(k, sks, exe=exe, env=None):
        """-> (se int16 [n, 2K * 256], copied pk records, ok list)"""
        count[0] += 1
        src, dst = str(workdir / ("in%d.bin" % count[0])), str(workdir / ("out%d.bin" % count[0]))
        with open(src, "wb") as f:
            f.write(b"".join(sks))
        r = subprocess.run([exe, str(k), src, dst], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env)
        assert r.returncode == 0, r.stdout[-3000:]
        out = open(dst, "rb").read()
        n, seb, pkb = len(sks), 2 * k * 512, 384 * k + 32
        assert len(out) == n * (seb + pkb + 1)
        se = np.frombuffer(out[:n * seb], np.int16).reshape(n, 2 * k * 256)
        pks = [out[n * seb + b * pkb:n * seb + (b + 1) * pkb] for b in range(n)]
        return se, pks, list(out[n * (seb + pkb):])
    return run


def test_python_model_is_the_key_generation():
    """NTT(s) of the key generation's s packs to the sk, the inverse undoes it, and the model's witness is the key generation's"""
    for k in KS:
        for i in range(2):
            pk, sk, s, e = kc.honest(k, i)
            assert b"".join(kc.pack12(kc.ntt(p)) for p in s) == sk[:384 * k]
            assert [kc.centred(kc.invntt(kc.ntt(p))) for p in s] == s
            assert kc.witness(k, sk) == (s, e)
            assert kc.key_from_witness(k, sk[768 * k:768 * k + 32], s, e, sk[-32:]) == (pk, sk)


def test_fixture_internal_checks():
    fx = kc.fixture()
    assert fx["format"] == "kosk-keyproof-v1" and fx["per_k"] == 2
    assert os.path.getsize(kc.FIXTURE) < 64 << 10
    for k in KS:
        items = fx["k"]["k%d" % k]
        assert len(items) == 2
        for it, (pk, sk) in zip(items, kc.foreign(k)):
            assert len(sk) == 768 * k + 96 and sk[384 * k:768 * k + 32] == pk
            assert hashlib.sha3_256(pk).hexdigest() == it["pk_sha3"] and sk[768 * k + 32:768 * k + 64] == hashlib.sha3_256(pk).digest()


def test_fixture_equals_reference():
    """the whole file again from oracle/_ref/libkyber_ref_k*.so"""
    missing = [p for p in (os.path.join(ROOT, "oracle", "_ref", "libkyber_ref_k%d.so" % k) for k in KS) if not os.path.exists(p)]
    if missing:
        if os.environ.get("KOSK_REQUIRE_REF") == "1":
            pytest.fail("KOSK_REQUIRE_REF=1 but %s is missing: run `make -C oracle` where the reference tree is mounted" % missing[0])
        return  # the internal checks above are what runs here
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        import make_keyproof_vectors
    finally:
        sys.path.pop(0)
    assert make_keyproof_vectors.build() == kc.fixture()


@pytest.mark.parametrize("k", KS)
def test_recovery_equals_the_key_generation(model, k):
    """8 seeds: s, e of api.host_keygen, ok = 1, the pk bytes copied; and the same with every s-hat field c < 767 stored as c + q"""
    keys = [kc.honest(k, i) for i in range(SEEDS)]
    folded = [kc.noncanonical_shat(k, sk) for _, sk, _, _ in keys]
    assert all(changed > 0 and sk2 != key[1] for (sk2, changed), key in zip(folded, keys))
    se, pks, ok = model(k, [key[1] for key in keys] + [sk2 for sk2, _ in folded])
    assert ok == [1] * (2 * SEEDS)
    for b in range(2 * SEEDS):
        pk, _, s, e = keys[b % SEEDS]
        assert se[b].tolist() == kc.se_rows(s, e), (k, b)
        assert pks[b] == pk
    # honest keys reach both ends of the range, so the accept edge of the check is exercised by them already
    eta = kc.ETA1[k]
    assert se[:SEEDS].max() == eta and se[:SEEDS].min() == -eta


@pytest.mark.parametrize("k", KS)
def test_foreign_keys_are_accepted(model, k):
    """key pairs of the reference's crypto_kem_keypair_derand: accepted, and t-hat = A o NTT(s) + NTT(e) holds in the Python model"""
    keys = kc.foreign(k)
    se, pks, ok = model(k, [sk for _, sk in keys])
    assert ok == [1, 1]
    for b, (pk, sk) in enumerate(keys):
        s = [se[b][256 * r:256 * (r + 1)].tolist() for r in range(k)]
        e = [se[b][256 * (k + r):256 * (k + r + 1)].tolist() for r in range(k)]
        assert kc.in_range(k, s, e) and (s, e) == kc.witness(k, sk)
        assert kc.key_from_witness(k, sk[768 * k:768 * k + 32], s, e, sk[-32:]) == (pk, sk)
        assert pks[b] == pk


@pytest.mark.parametrize("k", KS)
def test_range_edges(model, k):
    """every edge value as the sole defect of an otherwise honest key: +-eta1 accepted with the exact witness, +-(eta1 + 1), 1664 and
    1665 rejected with s, e all zero"""
    cases = kc.range_edges(k)
    assert len(cases) == 2 * 2 * 3 * 6 and sum(1 for c in cases if c[2]) == 24
    se, _, ok = model(k, [c[1] for c in cases])
    for b, (name, sk, accepted) in enumerate(cases):
        assert ok[b] == int(accepted), (k, name)
        if accepted:
            s, e = kc.witness(k, sk)
            assert se[b].tolist() == kc.se_rows(s, e), (k, name)
            target, i, j, value = name[0], int(name[2]), int(name.split("[")[2].split("]")[0]), int(name.split("=")[1])
            assert se[b][256 * ((k if target == "e" else 0) + i) + j] == value
        else:
            assert not se[b].any(), (k, name)


@pytest.mark.parametrize("k", KS)
def test_extreme_keys_and_pk_swap(model, k):
    ext = kc.extreme_keys(k)
    se, _, ok = model(k, [x[1] for x in ext] + [kc.pk_swapped(k)])
    assert ok == [1, 1, 0]
    for b, (_, _, s, e) in enumerate(ext):
        assert se[b].tolist() == kc.se_rows(s, e)
    assert kc.parse_sk(k, ext[1][1])[1] == [[0] * 256] * k  # s = e = 0: t = 0
    assert not se[2].any()
    assert not kc.in_range(k, *kc.witness(k, kc.pk_swapped(k)))


def test_sanitizer_run(model, workdir):
    """the host model as its own program under ASan + UBSan on the recovery vectors, the range edges and the rejected keys: every buffer
    of the program is a heap block of exactly the size of its device counterpart"""
    exe = _build(workdir, "witness_host_model_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    for k in KS:
        sks = [kc.honest(k, i)[1] for i in range(SEEDS)] + [kc.noncanonical_shat(k, kc.honest(k, 0)[1])[0]] + \
              [c[1] for c in kc.range_edges(k)[:12]] + [kc.pk_swapped(k)] + [x[1] for x in kc.extreme_keys(k)]
        se, _, ok = model(k, sks, exe=exe, env=env)
        plain = model(k, sks)
        assert ok == plain[2] and (se == plain[0]).all()


def test_oracle_proof_helper_reproduces_a_verifiable_keygen(oracle):
    """the helper the GPU tests compare foreign keys' proofs with: on the sk of the oracle's own verifiable key generation it gives that
    call's proof (so reading the tape from byte 64 on, and the ko_mlwe built from the recovered witness, are right)"""
    k = 2
    tape = oracle.tape_bytes_for(k, 5)
    _, sk, pi, _, _ = oracle.verifiable_keygen(k, tape)
    assert kc.oracle_proof(k, sk, tape) == pi
    assert kc.oracle_proof(k, sk, b"\xff" * 64 + tape[64:]) == pi


@pytest.mark.parametrize("k", KS)
def test_compat_header_compiles(k, workdir):
    """include/kosk_compat.hpp with kyber_kosk_prove_key used, syntax only (no example calls it)"""
    src = workdir / ("compat_k%d.cpp" % k)
    src.write_text('#include "kosk_compat.hpp"\nbool prove(const kyber_keypair *kp, uint8_t *pi) { return kyber_kosk_prove_key(kp, pi); }\n')
    r = subprocess.run(["c++", "-std=c++17", "-fsyntax-only", "-DKYBER_K=%d" % k, "-I", os.path.join(ROOT, "include"), str(src)],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
