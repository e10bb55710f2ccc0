"""What the head-signature tests share: the pinned seed and identifier, the golden file, the history whose 32 heads
the signing test signs, and the batch items of the verifier's tests.  Everything here is hashlib and tests/headsig_model.py; the golden
file tests/golden/headsig_v1.json is written by tests/golden/make_headsig_vectors.py."""
import functools
import hashlib
import json
import os

from tests import headsig_model as m
from tests import registry_history_model as hm

SEED = bytes(range(32))
ID = bytes(range(16))
OTHER_SEED = bytes(range(1, 33))
K = 2            # the handle's kyber_k in the GPU tests (the smallest keys)
GOLDEN_K = 3     # the kyber_k of the pinned signatures
H_SIGN = 5       # the signing test: 31 events, every size 0..31
CAPACITY = 32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "headsig_v1.json")


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def key(h, seed=SEED, key_id=ID):
    return m.Key(h, seed, key_id)


def golden_root(h, q):
    return hashlib.sha3_256(b"headsig golden root %d %d" % (h, q)).digest()


def pk_bytes(k):
    return 384 * k + 32


def event_key(k, tag, i):
    """any bytes of the right length are a key to kosk_registry_admit"""
    return hashlib.shake_256(b"headsig:%d:%d:%d" % (k, tag, i)).digest(pk_bytes(k))


@functools.lru_cache(maxsize=None)
def history(k, tag):
    """31 admissions into slots 0..30 -> (pks, the 32 heads of sizes 0..31)"""
    pks = [event_key(k, tag, i) for i in range(CAPACITY - 1)]
    log = hm.Log(k, CAPACITY)
    log.admit([(i, hashlib.sha3_256(p).digest()) for i, p in enumerate(pks)])
    assert len(log.events) == CAPACITY - 1
    return pks, [hm.mth(k, log.leaves(n)) for n in range(CAPACITY)]


def history_signatures(k, tag):
    """-> (signatures of sizes 0..31 under key(5), the set of coefficients the model saw)"""
    seen = set()
    _, heads = history(k, tag)
    return [key(H_SIGN).sign(k, heads[n], n, seen) for n in range(CAPACITY)], seen


def batch_root(tag, b):
    return hashlib.sha3_256(b"headsig batch root %d %d" % (tag, b)).digest()


def batch_items(k, tag, n):
    """n valid items under key(5): item b is the head (batch_root(tag, b), b % 32) -> (roots, sizes, sigs, coefficients seen)"""
    seen = set()
    roots = [batch_root(tag, b) for b in range(n)]
    sizes = [b % (1 << H_SIGN) for b in range(n)]
    sigs = [key(H_SIGN).sign(k, r, s, seen) for r, s in zip(roots, sizes)]
    return roots, sizes, sigs, seen
