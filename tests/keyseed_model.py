"""The model of format kosk-keyseed-v1, hashlib only and written from the format text -- tests only.

    seed = SHAKE256( "kosk-keyseed-v1" || 00            (16 bytes)
                  || LE32(K) || LE32(flags)             ( 8 bytes)
                  || context[32]                        (all zero unless flags bit 0)
                  || salt[32]                           (all zero unless flags bit 1)
                  || sk[768 K + 96] )[0 : 32]
    flags bit 0: the proof is context-bound; bit 1: a salt was given
    tape = kosk-seedtape-v1(seed):  SHAKE256(seed || "kosk-seedtape-v1" || LE32(K) || LE32(j))[0:136] for j = 0, 1, ..., cut to the tape length
"""
import hashlib
import json
import os
import struct

KS = (2, 3, 4)
LABEL = b"kosk-keyseed-v1\x00"
TAPE_LABEL = b"kosk-seedtape-v1"
TAPE_BYTES = {2: 65280, 3: 68062, 4: 75676}
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyseed_v1.json")
KEYS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "keyproof_keys_v1.json")
PIN_CONTEXT = bytes(range(32))                 # 00 .. 1f
PIN_SALT = bytes(255 - i for i in range(32))   # ff .. e0


def sk_bytes(k):
    return 768 * k + 96


def message(k, sk, context=None, salt=None):
    assert k in KS and len(sk) == sk_bytes(k) and len(LABEL) == 16
    assert context is None or len(context) == 32
    assert salt is None or len(salt) == 32
    flags = (1 if context is not None else 0) | (2 if salt is not None else 0)
    m = LABEL + struct.pack("<II", k, flags) + (bytes(context) if context is not None else bytes(32)) + (bytes(salt) if salt is not None else bytes(32)) + bytes(sk)
    assert len(m) == 88 + sk_bytes(k)
    return m


def seed(k, sk, context=None, salt=None):
    return hashlib.shake_256(message(k, sk, context, salt)).digest(32)


def tape_from_seed(k, s):
    assert len(s) == 32
    t = TAPE_BYTES[k]
    return b"".join(hashlib.shake_256(s + TAPE_LABEL + struct.pack("<II", k, j)).digest(136) for j in range(-(-t // 136)))[:t]


def shape(k):
    """(message bytes, Keccak-f count, bytes in the last block) of the sponge over the message"""
    n = 88 + sk_bytes(k)
    return n, n // 136 + 1, n % 136


def fixture_keys(k):
    with open(KEYS) as f:
        return [bytes.fromhex(it["sk"]) for it in json.load(f)["k"]["k%d" % k]]


def fixture():
    with open(FIXTURE) as f:
        return json.load(f)


def flag_cases():
    """the four flag combinations as (context, salt) of the pinned values"""
    return [(None, None), (PIN_CONTEXT, None), (None, PIN_SALT), (PIN_CONTEXT, PIN_SALT)]
