"""The inputs of tests/golden/kem_vectors_v1.json, shared by its generator (tests/golden/make_kem_vectors.py) and the tests that read it.

Keys: api.host_keygen(K, SHAKE256("kosk-kem-v1:kg:K:i", 64)) -- kyber_keygen of kosk.cpp:4-70, whose seed hashing differs from the
reference's keypair_derand, so that a test can regenerate every key pair without the reference; the fixture pins their SHA3-256.
Messages: m = SHAKE256("kosk-kem-v1:m:K:i", 32); item 0 all zero, item 1 all 0xFF.
Item 2 is encapsulated to a NON-CANONICAL encoding of its public key: every coefficient c < 767 stored as c + q (still 12 bits).
Item 3 also carries three tampered ciphertexts, one flipped bit each: byte 0, the last byte of the u part, the last byte.
"""
import functools
import hashlib
import json
import os

Q = 3329
ITEMS = 130
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kem_vectors_v1.json")
CT_BYTES = {2: 768, 3: 1088, 4: 1568}
U_BYTES = {2: 640, 3: 960, 4: 1408}  # 32 K d_u


def kg_seed(k, i):
    return hashlib.shake_256(b"kosk-kem-v1:kg:%d:%d" % (k, i)).digest(64)


def message(k, i):
    if i == 0:
        return bytes(32)
    if i == 1:
        return b"\xff" * 32
    return hashlib.shake_256(b"kosk-kem-v1:m:%d:%d" % (k, i)).digest(32)


def noncanonical_pk(pk, k):
    """every coefficient c < 4096 - q = 767 re-encoded as c + q; returns (pk', number of coefficients changed)"""
    body, changed = noncanonical_polyvec(pk[:384 * k])
    return body + pk[384 * k:], changed


def noncanonical_polyvec(body):
    """the same for any polyvec of 384 K bytes (t-hat of a pk, s-hat of an sk); returns (body', number of coefficients changed)"""
    assert len(body) % 384 == 0
    out = bytearray(body)
    changed = 0
    for t in range(len(body) // 3):  # 3 bytes hold two 12-bit coefficients (poly_tobytes, kyber/poly.c:128-147)
        b0, b1, b2 = out[3 * t:3 * t + 3]
        c = [b0 | ((b1 & 0x0F) << 8), (b1 >> 4) | (b2 << 4)]
        for j in range(2):
            if c[j] < 4096 - Q:
                c[j] += Q
                changed += 1
        out[3 * t:3 * t + 3] = bytes([c[0] & 0xFF, (c[0] >> 8) | ((c[1] & 0x0F) << 4), c[1] >> 4])
    return bytes(out), changed


def tamper_bytes(k):
    return [0, U_BYTES[k] - 1, CT_BYTES[k] - 1]


def tampered(ct, at):
    t = bytearray(ct)
    t[at] ^= 1
    return bytes(t)


@functools.lru_cache(maxsize=None)
def keypair(k, i):
    from mpcith_kyber_kosk_amd import api
    pk, sk = api.host_keygen(k, kg_seed(k, i))[:2]
    return pk, sk


def enc_pk(k, i):
    """the public key item i is encapsulated to"""
    pk = keypair(k, i)[0]
    return noncanonical_pk(pk, k)[0] if i == 2 else pk


@functools.lru_cache(maxsize=None)
def load():
    with open(PATH) as f:
        return json.load(f)


def sha3(b):
    return hashlib.sha3_256(b).hexdigest()
