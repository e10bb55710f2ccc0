"""KEM with one resident key, the parts that need no GPU: the five names and the three path ids are declared, bound
and exported, the NULL-argument returns, and tests/golden/kem_onekey_v1.json against hashlib, the older fixture and -- where oracle/_ref
is present -- the reference itself."""
import ctypes as C
import hashlib
import importlib.util
import json
import os
import re

import pytest

from tests import kem_fixture as kf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["kosk_kem_key_set", "kosk_kem_key_state", "kosk_kem_key_clear", "kosk_kem_enc_key", "kosk_kem_dec_key"]
FIXTURE = os.path.join(ROOT, "tests", "golden", "kem_onekey_v1.json")
KS = (2, 3, 4)


@pytest.fixture(scope="module")
def api():
    from mpcith_kyber_kosk_amd import api
    return api


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def _generator():
    spec = importlib.util.spec_from_file_location("make_kem_onekey_vectors", os.path.join(ROOT, "tests", "golden", "make_kem_onekey_vectors.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_names_are_declared_bound_and_exported(api):
    header = open(os.path.join(ROOT, "include", "kosk_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint %s\s*\((?:const )?kosk_ctx \*ctx" % name, code), name
        assert name in api.EXPORTS and hasattr(api.lib, name), name
        assert getattr(api.lib, name).argtypes is not None, name
    assert re.search(r"enum\s*\{\s*KOSK_KEM_KEY_NONE = 0,\s*KOSK_KEM_KEY_PK = 1,\s*KOSK_KEM_KEY_SK = 2\s*\}", code)
    assert (api.KEM_KEY_NONE, api.KEM_KEY_PK, api.KEM_KEY_SK) == (0, 1, 2)
    assert (api.Kosk.PATH_KEM_KEY_SETUP, api.Kosk.PATH_KEM_ENC_KEY, api.Kosk.PATH_KEM_DEC_KEY) == (19, 20, 21)
    for method in ("kem_key_set", "kem_key_state", "kem_key_clear", "kem_enc_key", "kem_dec_key"):
        assert callable(getattr(api.Kosk, method))
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int kosk_path_count\(", header, flags=re.S)
    assert m and re.search(r"\b19 launches of k_kem_key_setup\b", m.group(1)) and re.search(r"\b20 kem_enc_key / 21 kem_dec_key\b", m.group(1))


def test_null_arguments_return_minus_one(api):
    lib = api.lib
    buf = C.create_string_buffer(64)
    assert lib.kosk_kem_key_set(None, buf, None) == -1
    assert lib.kosk_kem_key_state(None) == -1
    assert lib.kosk_kem_key_clear(None) == -1
    assert lib.kosk_kem_enc_key(None, 1, buf, buf, buf) == -1
    assert lib.kosk_kem_dec_key(None, 1, buf, buf) == -1


def test_fixture_is_small_and_whole(fixture):
    assert os.path.getsize(FIXTURE) < 64 * 1024
    assert fixture["format"] == "kosk-kem-onekey-v1" and fixture["key"] == 3 and fixture["items"] == 130
    for k in KS:
        v = fixture["k"]["k%d" % k]
        assert len(v["ct"]) == len(v["ss"]) == 130 * 64 and len(v["tampered"]) == 3 and len(v["nc_pk"]) == 8 and len(v["nc_shat"]) == 8
        assert len(v["ct5_hex"]) == 2 * kf.CT_BYTES[k]


@pytest.mark.parametrize("k", KS)
def test_item_3_is_item_3_of_the_per_item_fixture(k, fixture):
    old = kf.load()["k"]["k%d" % k][3]
    assert _generator().items_of(fixture["k"]["k%d" % k])[3] == [old["ct"], old["ss"]]


@pytest.mark.parametrize("k", KS)
def test_rejection_keys_equal_hashlib(k, fixture):
    """every recorded rejection key is SHAKE256(z || ct) of item 5's ciphertext with that bit flipped; the dec digest equals the digest over
    the ss column (dec(ct) == ss for every canonical item); the non-canonical s-hat decapsulates to the canonical secrets"""
    v = fixture["k"]["k%d" % k]
    items = _generator().items_of(v)
    z = kf.keypair(k, 3)[1][-32:]
    ct5 = bytes.fromhex(v["ct5_hex"])
    assert kf.sha3(ct5) == items[5][0]
    assert [t["byte"] for t in v["tampered"]] == kf.tamper_bytes(k)
    for t in v["tampered"]:
        assert t["dec_ss"] == hashlib.shake_256(z + kf.tampered(ct5, t["byte"])).digest(32).hex()
    assert v["dec"] == kf.sha3(b"".join(bytes.fromhex(it[1]) for it in items))
    assert v["nc_shat"] == [it[1] for it in items[:8]]
    assert all(a != b for a, b in zip(v["nc_pk"], items))


def test_fixture_regenerates_from_the_reference(fixture):
    if not os.path.exists(os.path.join(ROOT, "oracle", "_ref", "libkyber_ref_k3.so")):
        return  # the reference's binaries are not part of a checkout: nothing to compare with
    gen = _generator()
    assert gen.dump(gen.build()) == open(FIXTURE).read()
