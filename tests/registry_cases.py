"""Shared pieces of the registry tests: the slot maps and the helpers that compare kosk_kem_enc_slots with
tests/golden/kem_vectors_v1.json -- what the reference's crypto_kem_enc_derand returned for 130 distinct keys -- and kosk_registry_read
with hashlib.  Every comparison is exact."""
import functools
import hashlib

from tests import kem_fixture as kf

KS = (2, 3, 4)
CHUNK = 16384  # KEM_CHUNK of csrc/kosk_ctx.hpp: items per launch group
WAVE_MAX = 1024  # KEM_WAVE_MAX: up to this many keys an admission runs K^2 + 1 one-wave blocks per key, above it one sponge per lane

CAPACITY = 300
EDGE_CAPACITY = 1100
BIG_CAPACITY = 16400


def slot(i):
    """fixture item i -> its slot in a registry of 300: injective (gcd(37, 300) = 1); item 97 on slot 0, item 24 on slot 299"""
    return (37 * i + 11) % CAPACITY


def edge_slot(b):
    """key b of the layout-edge admissions (up to 1 025 keys, capacity 1 100): injective (gcd(7, 1100) = 1)"""
    return (7 * b + 5) % EDGE_CAPACITY


def big_slot(b):
    """key b of the launch-group admission (16 385 keys, capacity 16 400): injective (gcd(7, 16400) = 1)"""
    return (7 * b + 3) % BIG_CAPACITY


@functools.lru_cache(maxsize=None)
def pks(k):
    """the 130 public keys the fixture's items are encapsulated to (item 2: the non-canonical encoding) -- computed once, never modified"""
    return tuple(kf.enc_pk(k, i) for i in range(kf.ITEMS))


@functools.lru_cache(maxsize=None)
def messages(k):
    return tuple(kf.message(k, i) for i in range(kf.ITEMS))


def items(k):
    return kf.load()["k"]["k%d" % k]


def admit_fixture(ctx, k, capacity=CAPACITY):
    """a registry of `capacity` slots with fixture key i in slot(i)"""
    ctx.registry_reserve(capacity)
    ctx.registry_admit(list(pks(k)), [slot(i) for i in range(kf.ITEMS)])
    assert ctx.registry_level() == (kf.ITEMS, capacity)


def check_enc(ctx, k, idx, slots):
    """kosk_kem_enc_slots on `slots` with the messages of fixture items `idx`: every ct digest, ss and done bit against the fixture"""
    cts, sss, done = ctx.kem_enc_slots(slots, [messages(k)[i] for i in idx])
    want = items(k)
    assert done == [True] * len(idx)
    for b, i in enumerate(idx):
        assert kf.sha3(cts[b]) == want[i]["ct"], ("ct", k, b, i)
        assert sss[b].hex() == want[i]["ss"], ("ss", k, b, i)
    return cts, sss


def check_read(ctx, k, idx, slots):
    """kosk_registry_read of `slots`, which hold the keys of fixture items `idx`: occupied, the pk bytes, hashlib's SHA3-256 of them"""
    states, got_pk, got_h = ctx.registry_read(slots)
    assert states == [1] * len(idx)
    for b, i in enumerate(idx):
        assert got_pk[b] == pks(k)[i], ("pk", k, b, i)
        assert got_h[b] == hashlib.sha3_256(pks(k)[i]).digest(), ("h", k, b, i)


def inst(api, k, seed64):
    """the mlwe_inst image (A, t, s, e) of kyber_keygen on seed64 (kosk_verify_inst: a verify call that leaves no pk bytes in HBM)"""
    pk, sk, A, s, e, t = api.host_keygen(k, seed64)
    return A.tobytes() + t.tobytes() + s.tobytes() + e.tobytes()


def counts(ctx, api):
    """the registry's two counters, the per-item and one-key encapsulation counters, k_wipe, and the level"""
    ids = (api.Kosk.PATH_REGISTRY_ADMIT, api.Kosk.PATH_KEM_ENC_SLOTS, 12, 20, api.Kosk.PATH_WIPE)
    return tuple(ctx.path_count(i) for i in ids) + ctx.registry_level()
