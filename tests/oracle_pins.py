"""The oracle's outputs per (Kyber K, tape index), pinned in tests/golden/oracle_batch_pins_v1.json (tests/golden/make_oracle_pins.py
writes it): lets a GPU test compare EVERY position of a large batch with the oracle without running the oracle on every tape.

    mism = oracle_pins.check(k, tape_indices, pks, sks, pis)       # [] or every mismatching position, and which of pk / sk / pi
    oracle_pins.assert_batch(k, tape_indices, pks, sks, pis)       # the same, as one AssertionError that lists them all
"""
import base64
import functools
import hashlib
import json
import os

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "oracle_batch_pins_v1.json")
FIELDS = ("pk", "sk", "pi", "h1", "ch")


@functools.lru_cache(maxsize=None)
def _raw():
    with open(PATH) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def table(k):
    """{tape index: {"pk", "sk", "pi", "h1", "ch": truncated digest bytes}} of one K"""
    ent = _raw()["k%d" % k]
    nb = _raw()["digest_bytes"]
    blobs = {f: base64.b64decode(ent[f]) for f in FIELDS}
    idxs = [s + i for s, c in ent["ranges"] for i in range(c)]
    for f in FIELDS:
        assert len(blobs[f]) == nb[f] * len(idxs), (k, f)
    return {idx: {f: blobs[f][p * nb[f]:(p + 1) * nb[f]] for f in FIELDS} for p, idx in enumerate(idxs)}


def features(k, idx):
    """the tape's rare content features: alpha values among {0, 1, q - 1}, and the most SHAKE128 blocks any gen_matrix entry needed"""
    ent = _raw()["k%d" % k]
    return {"alpha_edge": ent["alpha_edge"].get(str(idx), []), "xof_blocks": ent["xof_blocks"].get(str(idx), 3)}


def rare_tapes(k):
    """tape indices with an alpha edge value or a fourth XOF block"""
    ent = _raw()["k%d" % k]
    return sorted({int(i) for i in ent["alpha_edge"]} | {int(i) for i in ent["xof_blocks"]})


def missing(k, tape_indices):
    t = table(k)
    return sorted({i for i in tape_indices if i not in t})


def _d(x, n):
    return hashlib.sha3_256(x).digest()[:n]


def check(k, tape_indices, pks=None, sks=None, pis=None):
    """[(position, tape index, [differing fields])] over every position of the batch; pks / sks / pis may be None (not compared)"""
    t = table(k)
    nb = _raw()["digest_bytes"]
    counts = [(f, len(xs)) for f, xs in (("pk", pks), ("sk", sks), ("pi", pis)) if xs is not None and len(xs) != len(tape_indices)]
    if counts:
        return [(None, None, ["%s: %d outputs for %d tapes" % (f, c, len(tape_indices)) for f, c in counts])]
    out = []
    for b, idx in enumerate(tape_indices):
        pin = t[idx]
        bad = [f for f, xs in (("pk", pks), ("sk", sks), ("pi", pis)) if xs is not None and _d(xs[b], nb[f]) != pin[f]]
        if bad:
            out.append((b, idx, bad))
    return out


def check_tables(k, tape_indices, tcomm, views):
    """the resident digest tables of a batch ([n][1454][32] uint8 arrays, either may be None) against the pinned h1 / ch:
    [(position, tape index, [differing tables])]"""
    t = table(k)
    nb = _raw()["digest_bytes"]
    out = []
    for b, idx in enumerate(tape_indices):
        bad = [f for f, tab in (("h1", tcomm), ("ch", views)) if tab is not None and _d(tab[b].tobytes(), nb[f]) != t[idx][f]]
        if bad:
            out.append((b, idx, bad))
    return out


def _fail(what, k, tape_indices, mism):
    if mism:
        raise AssertionError("%s: %d of %d positions differ from the oracle pins (K=%d), (position, tape, fields): %s" %
                             (what, len(mism), len(tape_indices), k, mism))


def assert_batch(k, tape_indices, pks=None, sks=None, pis=None, what="batch"):
    _fail(what, k, tape_indices, check(k, tape_indices, pks, sks, pis))


def assert_tables(k, tape_indices, tcomm, views, what="digest tables"):
    _fail(what, k, tape_indices, check_tables(k, tape_indices, tcomm, views))
