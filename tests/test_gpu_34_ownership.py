"""Buffer ownership: the inventory allocates, lists and frees every buffer, and a cohort member is built by rule from the three
parts of the context.  Nothing a caller can see changed, so every expectation here was taken from the commit before: what a cohort member
accepts, the bytes of the proofs, and the secret regions of tests/golden/inventory_regions.json.  K = 2 and max_batch = 2 throughout (the
golden numbers: K = 2, 3, 4).  Cases with several handles run in a fresh child process (tests/gpu_child_ownership.py)."""
import json
import os

import pytest

from tests import bank_cases as bc
from tests import kem_fixture as kf

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, MAX_BATCH = 2, 2

# what member 1 of a cohort of three answered to each per-handle call on the commit before ("ok": accepted), and what it then reported
MEMBER_CALLS = {"bank_reserve": "ok", "compact_fetch": "ok", "kem_key_set": "ok", "registry_reserve": "ok", "set_contexts": "ok", "transcode": "ok",
                "witness_from_sk": "ok"}
MEMBER_STATE = {"bank": 2, "kem_key_state": 1, "registry": 4}


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return torch


@pytest.fixture()
def handle(torch_cuda):
    from mpcith_kyber_kosk_amd import api
    h = api.Kosk(kyber_k=K, max_batch=MAX_BATCH)
    yield h
    h.close()


def _line(out, tag):
    return json.loads(next(ln for ln in out.splitlines() if ln.startswith(tag + " "))[len(tag) + 1:])


def test_cohort_isolation(gpu_child, torch_cuda):
    """key slot, registry, bank, armed contexts, compact staging, transcode workspace and witness buffers on member 1 only: accepted as
    before, members 0 and 2 keep an empty slot, capacity 0 and all-zero path counters, and all three then prove and verify the bytes of an
    uncombined handle"""
    out = gpu_child("from tests.gpu_child_ownership import cohort_isolation; cohort_isolation()", timeout=240)
    assert _line(out, "outcomes") == MEMBER_CALLS
    assert _line(out, "member1") == MEMBER_STATE
    assert "cohort_isolation ok" in out


def test_teardown_orders(gpu_child, torch_cuda):
    out = gpu_child("from tests.gpu_child_ownership import teardown_orders; teardown_orders()", timeout=240)
    assert "teardown_orders ok" in out


def test_inventory_numbers_are_the_parents(gpu_child, torch_cuda):
    """bytes and regions of the secret HBM regions in three states, of a plain handle and of a cohort member, at K = 2, 3, 4"""
    with open(os.path.join(ROOT, "tests", "golden", "inventory_regions.json")) as f:
        want = json.load(f)["numbers"]
    out = gpu_child("from tests.gpu_child_ownership import inventory_numbers; inventory_numbers()", timeout=300)
    got = _line(out, "inventory")
    print(json.dumps(got, sort_keys=True))
    assert got == want


def test_kem_workspace_regrows(handle):
    """n = 1, then n = 1025 on the same handle: the workspace holds 1 024 items after the first call and is wiped, freed and allocated
    again for the second; every position equals the fixture the KEM tests compare against"""
    items = kf.load()["k"]["k%d" % K]
    for n in (1, 1025):
        idx = [b % kf.ITEMS for b in range(n)]
        cts, sss = handle.kem_enc([kf.enc_pk(K, i) for i in idx], [kf.message(K, i) for i in idx])
        assert [kf.sha3(c) for c in cts] == [items[i]["ct"] for i in idx], n
        assert [s.hex() for s in sss] == [items[i]["ss"] for i in idx], n


def test_witness_buffers_regrow(torch_cuda):
    """n = 1, then n = 3: the buffers of the first call are wiped, freed and allocated again.  kosk_witness_from_sk takes at most max_batch
    keys per call, so this one case runs on handles of max_batch = 3"""
    import numpy as np
    from mpcith_kyber_kosk_amd import api
    sks = bc.sks(K, 3)
    fresh, handle = api.Kosk(kyber_k=K, max_batch=3), api.Kosk(kyber_k=K, max_batch=3)
    want, ok = fresh.witness_from_sk(sks)
    fresh.close()
    assert ok == [True] * 3 and want.any()
    se1, ok1 = handle.witness_from_sk(sks[:1])
    assert ok1 == [True] and np.array_equal(se1, want[:1])
    se3, ok3 = handle.witness_from_sk(sks)
    assert ok3 == [True] * 3 and np.array_equal(se3, want)
    handle.close()


def test_bank_reserved_again(handle):
    """2 -> 0 -> 3, then a fill and a take: the proofs of kosk_prove_keys_batch on the same tapes"""
    tapes, sks = [bc.tape(K, 30 + i) for i in range(2)], bc.sks(K, 2)
    want, _ = handle.prove_keys(sks, tapes=tapes)
    handle.bank_reserve(2)
    assert handle.bank_level() == (0, 2)
    handle.bank_reserve(0)
    assert handle.bank_level() == (0, 0)
    handle.bank_reserve(3)
    assert handle.bank_level() == (0, 3)
    handle.bank_fill(tapes=tapes)
    assert handle.bank_level() == (2, 3)
    got, ok = handle.prove_keys_banked(sks, tapes=tapes)
    assert ok == [True] * 2 and got == want and handle.bank_level() == (0, 3)


def test_registry_reserved_again(handle):
    """4 -> 0 -> 8, then an admission into slots only the last reservation has, and a read of them"""
    import hashlib
    pks = bc.pks(K, 2)
    handle.registry_reserve(4)
    assert handle.registry_level() == (0, 4)
    handle.registry_reserve(0)
    assert handle.registry_level() == (0, 0)
    handle.registry_reserve(8)
    assert handle.registry_level() == (0, 8)
    handle.registry_admit(pks, [5, 7])
    assert handle.registry_level() == (2, 8)
    states, got, hs = handle.registry_read([5, 6, 7])
    assert states == [1, 0, 1] and got == [pks[0], bytes(len(pks[0])), pks[1]]
    assert hs == [hashlib.sha3_256(pks[0]).digest(), bytes(32), hashlib.sha3_256(pks[1]).digest()]
    handle.registry_evict([5, 7])
    handle.registry_reserve(0)
