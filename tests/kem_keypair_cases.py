"""The inputs of tests/golden/kem_keypair_v1.json and the models of the key-pair and key-check calls, shared by the fixture's generator
(tests/golden/make_kem_keypair_vectors.py) and the tests that read it.  Nothing here runs code of kosk_kem_keypair_batch or the checks.

Coins: SHAKE256("kosk-keypair-v1:K:i", 64) = d || z, i < ITEMS.
Key pair model: api.host_keygen (kosk_keygen, the host restatement of kosk.cpp:4-70, pinned to the reference elsewhere) hashes d || K
exactly as indcpa_keypair_derand does and differs from crypto_kem_keypair_derand only in the last 32 bytes of the sk, where it stores the
noise seed instead of z.
Flag model: a 12-bit decode and hashlib.
"""
import functools
import hashlib
import json
import os

from tests import kem_edges as ke

Q = 3329
ITEMS = 130
KS = (2, 3, 4)
HASH, PK_RANGE, S_RANGE = 1, 2, 4  # KOSK_KEYCHK_*
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kem_keypair_v1.json")


def coins(k, i):
    return hashlib.shake_256(b"kosk-keypair-v1:%d:%d" % (k, i)).digest(64)


def labelled(label, n):
    return hashlib.shake_256(b"kosk-keypair-v1:" + label).digest(n)


@functools.lru_cache(maxsize=None)
def _model(k, c):
    from mpcith_kyber_kosk_amd import api
    pk, sk0 = api.host_keygen(k, c)[:2]
    return pk, sk0[:-32] + c[32:]


def model(k, c):
    """(pk, sk) of crypto_kem_keypair_derand(coins = d || z)"""
    return _model(k, bytes(c))


def keypair(k, i):
    return model(k, coins(k, i))


def needs_fourth_block(k, c):
    """whether an entry of the key's matrix needs a fourth SHAKE128 block (A and A^T hold the same entries)"""
    return any(s[0] >= 4 for s in ke.matrix_stats(k, ke.rho_of_seed(k, c)))


def fields(body):
    """the 12-bit fields of a polyvec's bytes (poly_tobytes, kyber/poly.c:128-147)"""
    out = []
    for t in range(len(body) // 3):
        b0, b1, b2 = body[3 * t:3 * t + 3]
        out += [b0 | ((b1 & 0x0F) << 8), (b1 >> 4) | (b2 << 4)]
    return out


def set_field(rec, at, index, value):
    """rec with 12-bit field `index` of the polyvec that starts at byte `at` set to value"""
    out = bytearray(rec)
    p = at + 3 * (index // 2)
    if index % 2 == 0:
        out[p] = value & 0xFF
        out[p + 1] = (out[p + 1] & 0xF0) | (value >> 8)
    else:
        out[p + 1] = (out[p + 1] & 0x0F) | ((value & 0x0F) << 4)
        out[p + 2] = value >> 4
    return bytes(out)


def flip(rec, byte, bit=None):
    out = bytearray(rec)
    out[byte] ^= 1 << (byte % 8 if bit is None else bit)
    return bytes(out)


def flags_pk(k, pk):
    return PK_RANGE if any(c >= Q for c in fields(pk[:384 * k])) else 0


def flags_sk(k, sk):
    pvb = 384 * k
    pk = sk[pvb:2 * pvb + 32]
    f = S_RANGE if any(c >= Q for c in fields(sk[:pvb])) else 0
    f |= flags_pk(k, pk)
    if hashlib.sha3_256(pk).digest() != sk[2 * pvb + 32:2 * pvb + 64]:
        f |= HASH
    return f


def sha3(b):
    return hashlib.sha3_256(b).hexdigest()


@functools.lru_cache(maxsize=None)
def load():
    with open(PATH) as f:
        return json.load(f)
