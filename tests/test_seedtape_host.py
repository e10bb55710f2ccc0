"""CPU tests of seeded proving's host side (include/kosk_mi355x.h: format kosk-seedtape-v1): kosk_tape_from_seed against the
hashlib construction and the committed anchors, argument errors of the handle-free calls, and the sanitizer builds of the host code
(which now carry tape_from_seed).  The device side is tests/test_gpu_13_seeded.py."""
import ctypes as C
import hashlib
import json
import os
import random
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LABEL = b"kosk-seedtape-v1"


def hashlib_tape(k, seed, tape_bytes):
    """the normative definition, with hashlib only"""
    nb = -(-tape_bytes // 136)
    return b"".join(hashlib.shake_256(seed + LABEL + struct.pack("<II", k, j)).digest(136) for j in range(nb))[:tape_bytes]


@pytest.fixture(scope="module")
def api():
    from mpcith_kyber_kosk_amd import api as a
    return a


@pytest.mark.parametrize("k", [2, 3, 4])
def test_tape_from_seed_equals_hashlib_construction(api, k):
    rng = random.Random(0x5eed0000 + k)
    seeds = [bytes(rng.getrandbits(8) for _ in range(32)) for _ in range(20)] + [bytes(32), b"\xff" * 32]
    t = api.tape_bytes(k)
    assert len(LABEL) == 16 and t == {2: 65280, 3: 68062, 4: 75676}[k]
    for seed in seeds:
        got = api.tape_from_seed(k, seed)
        assert len(got) == t
        assert got == hashlib_tape(k, seed, t), seed.hex()
    assert len({api.tape_from_seed(k, s) for s in seeds}) == len(seeds)


def test_tape_from_seed_writes_exactly_tape_bytes(api):
    for k in (2, 3, 4):
        t = api.tape_bytes(k)
        buf = C.create_string_buffer(b"\xa5" * (t + 256), t + 256)
        assert api.lib.kosk_tape_from_seed(k, C.c_char_p(bytes(range(32))), buf) == 0
        assert buf.raw[t:] == b"\xa5" * 256 and buf.raw[:t] == hashlib_tape(k, bytes(range(32)), t)


def test_anchors_of_the_committed_fixture(api):
    with open(os.path.join(ROOT, "tests", "golden", "seedtape_v1.json")) as f:
        fx = json.load(f)
    assert fx["format"] == "kosk-seedtape-v1"
    seed = bytes.fromhex(fx["seed"])
    assert seed == bytes(range(32))
    for k in (2, 3, 4):
        a = fx["anchors"]["k%d" % k]
        tape = api.tape_from_seed(k, seed)
        assert len(tape) == a["tape_bytes"] == api.tape_bytes(k) and a["blocks"] == -(-len(tape) // 136)
        assert hashlib.sha3_256(tape).hexdigest() == a["sha3_256"]
        assert tape[:8].hex() == a["head"] and tape[-4:].hex() == a["tail"]
        # the fixture itself against hashlib (it is written by tests/golden/make_seedtape_vectors.py, hashlib only)
        assert hashlib.sha3_256(hashlib_tape(k, seed, a["tape_bytes"])).hexdigest() == a["sha3_256"]


def test_fixture_generator_reproduces_the_committed_file(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_seedtape_vectors", os.path.join(ROOT, "tests", "golden", "make_seedtape_vectors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with open(os.path.join(ROOT, "tests", "golden", "seedtape_v1.json")) as f:
        fx = json.load(f)
    for k in (2, 3, 4):
        tape = mod.tape_from_seed(k, bytes.fromhex(fx["seed"]))
        assert len(tape) == mod.tape_bytes(k) == fx["anchors"]["k%d" % k]["tape_bytes"]
        assert hashlib.sha3_256(tape).hexdigest() == fx["anchors"]["k%d" % k]["sha3_256"]


def test_argument_errors_without_a_handle(api):
    lib = api.lib
    out = C.create_string_buffer(80000)
    for k in (-1, 0, 1, 5, 768):
        assert lib.kosk_tape_from_seed(k, C.c_char_p(bytes(32)), out) == -1
        with pytest.raises(api.KoskError):
            api.tape_from_seed(k, bytes(32))
    assert lib.kosk_tape_from_seed(3, None, out) == -1 and lib.kosk_tape_from_seed(3, C.c_char_p(bytes(32)), None) == -1
    with pytest.raises(api.KoskError):
        api.tape_from_seed(3, bytes(31))
    # kosk_set_entropy: a NULL handle is refused for every mode (modes other than 0 / 1 on a live handle: tests/test_gpu_13_seeded.py)
    for mode in (api.ENTROPY_TAPE, api.ENTROPY_SEED, 2, -1):
        assert lib.kosk_set_entropy(None, mode) == -1
    assert (api.ENTROPY_TAPE, api.ENTROPY_SEED, api.SEED_BYTES) == (0, 1, 32)


def test_new_entry_points_are_declared_and_exported(api):
    with open(os.path.join(ROOT, "include", "kosk_mi355x.h")) as f:
        hdr = f.read()
    for name in ("kosk_tape_from_seed", "kosk_tape_expand_device", "kosk_set_entropy", "kosk_verifiable_keygen_seeded_batch",
                 "kosk_verifiable_keygen_seeded_batch_compact", "kosk_verifiable_keygen_seeded_resident", "kosk_stage_prover_inputs_seeded"):
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib, name)
    assert "#define KOSK_SEED_BYTES 32" in hdr and "KOSK_ENTROPY_TAPE = 0, KOSK_ENTROPY_SEED = 1" in hdr
    assert api.Kosk.PATH_IDS.index("tape_expand") == 11  # appended: the existing ids keep their numbers


@pytest.mark.parametrize("target", ["asan", "tsan"])
def test_sanitizer_host_builds_still_build(target):
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "--no-print-directory", target], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-3000:]
