"""CPU tests of format kosk-keyseed-v1: kosk_keyseed_value (csrc/kosk_host.cpp, no GPU) against the fixture
tests/golden/keyseed_v1.json and the hashlib model tests/keyseed_model.py that wrote it."""
import ctypes as C
import hashlib
import os

import pytest

from tests import keyseed_model as km

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kosk_keyseed_value", "kosk_keyseed_device", "kosk_stage_prover_keys_derived", "kosk_prove_keys_derived_batch"]


@pytest.fixture(scope="module")
def api():
    from mpcith_kyber_kosk_amd import api as a
    return a


def _flip(b, byte, bit=0):
    return b[:byte] + bytes([b[byte] ^ (1 << bit)]) + b[byte + 1:]


def test_model_shapes_are_the_format_text():
    """88-byte header; 1720 / 2488 / 3256 message bytes; 13 / 19 / 24 permutations; last blocks of 88 / 40 / 128 bytes"""
    assert [km.shape(k) for k in km.KS] == [(1720, 13, 88), (2488, 19, 40), (3256, 24, 128)]
    m = km.message(3, bytes(km.sk_bytes(3)), km.PIN_CONTEXT, km.PIN_SALT)
    assert m[:16] == b"kosk-keyseed-v1\x00" and m[16:24] == bytes([3, 0, 0, 0, 3, 0, 0, 0])
    assert m[24:56] == bytes(range(32)) and m[56:88] == bytes(range(255, 223, -1))
    assert km.message(3, bytes(km.sk_bytes(3)))[16:88] == bytes([3, 0, 0, 0, 0, 0, 0, 0]) + bytes(64)


def test_fixture_is_what_the_model_writes():
    fx = km.fixture()
    assert fx["format"] == "kosk-keyseed-v1" and bytes.fromhex(fx["context"]) == km.PIN_CONTEXT and bytes.fromhex(fx["salt"]) == km.PIN_SALT
    seen = set()
    for k in km.KS:
        part = fx["k"]["k%d" % k]
        assert (part["message_bytes"], part["permutations"], part["last_block_bytes"]) == km.shape(k)
        keys = km.fixture_keys(k)
        assert len(part["vectors"]) == 4 * len(keys)
        for v in part["vectors"]:
            context = km.PIN_CONTEXT if v["flags"] & 1 else None
            salt = km.PIN_SALT if v["flags"] & 2 else None
            s = km.seed(k, keys[v["key"]], context, salt)
            assert s.hex() == v["seed"]
            assert hashlib.sha3_256(km.tape_from_seed(k, s)).hexdigest() == v["tape_sha3_256"]
            seen.add(v["seed"])
        assert sorted({v["flags"] for v in part["vectors"]}) == [0, 1, 2, 3]
    assert len(seen) == sum(len(fx["k"]["k%d" % k]["vectors"]) for k in km.KS)  # every seed differs from every other


@pytest.mark.parametrize("k", km.KS)
def test_keyseed_value_against_the_fixture_and_the_model(k, api):
    keys = km.fixture_keys(k)
    for v in km.fixture()["k"]["k%d" % k]["vectors"]:
        context = km.PIN_CONTEXT if v["flags"] & 1 else None
        salt = km.PIN_SALT if v["flags"] & 2 else None
        got = api.keyseed_value(k, keys[v["key"]], context, salt)
        assert got.hex() == v["seed"], (k, v["key"], v["flags"])
        assert hashlib.sha3_256(api.tape_from_seed(k, got)).hexdigest() == v["tape_sha3_256"]
    # one flipped bit in sk[0], the last sk byte, the context and the salt: the model's seed, and another than before
    sk = keys[0]
    base = api.keyseed_value(k, sk, km.PIN_CONTEXT, km.PIN_SALT)
    variants = [(_flip(sk, 0), km.PIN_CONTEXT, km.PIN_SALT), (_flip(sk, len(sk) - 1, 7), km.PIN_CONTEXT, km.PIN_SALT),
                (sk, _flip(km.PIN_CONTEXT, 31, 7), km.PIN_SALT), (sk, km.PIN_CONTEXT, _flip(km.PIN_SALT, 0))]
    seeds = {base}
    for s_, c_, t_ in variants:
        got = api.keyseed_value(k, s_, c_, t_)
        assert got == km.seed(k, s_, c_, t_)
        seeds.add(got)
    assert len(seeds) == 5


@pytest.mark.parametrize("k", km.KS)
def test_flags_separate_a_zero_field_from_a_missing_one(k, api):
    sk = km.fixture_keys(k)[1]
    zero = bytes(32)
    a, b = api.keyseed_value(k, sk), api.keyseed_value(k, sk, context=zero)
    c, d = api.keyseed_value(k, sk, salt=zero), api.keyseed_value(k, sk, zero, zero)
    assert len({a, b, c, d}) == 4
    assert (a, b, c, d) == (km.seed(k, sk), km.seed(k, sk, zero), km.seed(k, sk, None, zero), km.seed(k, sk, zero, zero))


def test_return_codes(api):
    lib = api.lib
    out = C.create_string_buffer(32)
    sk = C.c_char_p(bytes(km.sk_bytes(4)))
    for k in (1, 5, 0, -1):
        assert lib.kosk_keyseed_value(k, sk, None, None, out) == -1
    for k in km.KS:
        assert lib.kosk_keyseed_value(k, None, None, None, out) == -1
        assert lib.kosk_keyseed_value(k, sk, None, None, None) == -1
        assert lib.kosk_keyseed_value(k, sk, None, None, out) == 0
        assert out.raw == km.seed(k, bytes(km.sk_bytes(k)))
    with pytest.raises(api.KoskError):
        api.keyseed_value(3, bytes(km.sk_bytes(3) - 1))
    with pytest.raises(api.KoskError):
        api.keyseed_value(3, bytes(km.sk_bytes(3)), context=bytes(31))
    with pytest.raises(api.KoskError):
        api.keyseed_value(3, bytes(km.sk_bytes(3)), salt=bytes(33))
    # the handle calls refuse a NULL handle before anything else
    assert lib.kosk_keyseed_device(None, 1, sk, None, 0, None, 0, None) == -1
    assert lib.kosk_stage_prover_keys_derived(None, 1, sk, None, 0, out) == -1
    assert lib.kosk_prove_keys_derived_batch(None, 1, sk, None, 0, out, out) == -1


def test_new_entry_points_are_declared_and_exported(api):
    with open(os.path.join(ROOT, "include", "kosk_mi355x.h")) as f:
        hdr = f.read()
    for name in NAMES:
        assert name + "(" in hdr and name in api.EXPORTS and hasattr(api.lib, name), name
    assert api.Kosk.PATH_KEYSEED == 17 and api.Kosk.PATH_KEM_CHECK == 16  # appended: the existing ids keep their numbers
    with open(os.path.join(ROOT, "include", "kosk_compat.hpp")) as f:
        assert "kyber_kosk_prove_key_derived(" in f.read()
