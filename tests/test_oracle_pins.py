"""CPU: tests/golden/oracle_batch_pins_v1.json, the oracle digests every position of the GPU tests' batches is compared with
(tests/oracle_pins.py) -- it covers every tape those tests read, a seeded sample of it (rare content features of every K among
them) recomputes with the oracle, its tape-0 entries agree with kosk_tape_v1.json, and the rare features really occur."""
import concurrent.futures as cf
import importlib.util
import json
import os
import sys

import numpy as np

from tests import oracle_lib as oracle
from tests import oracle_pins

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_RARE = 3   # tapes per K and rare feature the fixture must hold


def _generator():
    spec = importlib.util.spec_from_file_location("make_oracle_pins", os.path.join(ROOT, "tests", "golden", "make_oracle_pins.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def gpu_test_tapes():
    """{K: tape indices} the GPU tests read in batches, by the formulas the tests use"""
    from tests import test_gpu_12_batch_positions as t12
    need = {k: set(v) for k, v in t12.pinned_tapes().items()}
    need[2] |= set(range(46))                              # test_gpu_08: config 2
    need[3] |= set(range(512)) | set(range(100, 164))      # test_gpu_04: config 5; test_gpu_07: 64-proof batch
    need[4] |= set(range(2000, 2091))                      # test_gpu_04: config 4
    # gpu_child_cases
    for k, n in ((3, 46), (4, 91), (3, 130)):              # big_batches
        need[k] |= set(range(1000, 1000 + n))
    for k, threads, rounds in ((2, 6, 4), (3, 6, 4), (4, 6, 4), (3, 5, 3)):   # combined_calls
        need[k] |= {5000 + (t * rounds + r) * 3 + b for t in range(threads) for r in range(rounds) for b in range(3)}
    for callers, rounds in ((6, 3), (4, 3), (3, 3), (16, 2)):                # line_of_record_shape
        need[3] |= {20000 + (t * rounds + r) * 46 + b for t in range(callers) for r in range(rounds) for b in range(46)}
    need[3] |= set(range(7000, 7007)) | {7100 + t * 3 + b for t in (1, 2) for b in range(3)}   # member_big_batch_stays_in_its_block
    need[2] |= {9500 + t * 3 + b for t in range(3) for b in range(3)}                         # cohort_round_hooks
    need[3] |= {9000 + t * 2 + b for t in range(5) for b in range(2)}                         # combined_members_come_and_go
    return need


def test_fixture_covers_every_gpu_batch():
    for k, idxs in gpu_test_tapes().items():
        assert oracle_pins.missing(k, idxs) == [], k
    assert os.path.getsize(oracle_pins.PATH) < 160 * 1024


def test_sample_recomputes_with_the_oracle():
    """about 40 seeded tapes -- a few of every rare feature per K, the rest plain -- recomputed: digests, alpha edge values and XOF
    block counts; the block counts of the rare ones also against the lane-level model of the kernel's wave sponge"""
    gen = _generator()
    rng = np.random.default_rng(20260)
    sample = []
    for k in (2, 3, 4):
        raw = oracle_pins._raw()["k%d" % k]
        edge = sorted(int(i) for i in raw["alpha_edge"])
        xof = sorted(int(i) for i in raw["xof_blocks"])
        plain = sorted(set(oracle_pins.table(k)) - set(edge) - set(xof))
        for pool, m in ((edge, 3), (xof, 3), (plain, 7)):
            sample += [(k, int(i)) for i in rng.choice(pool, min(m, len(pool)), replace=False)]
    oracle.verifiable_keygen(2, oracle.tape_bytes_for(2, 0))  # the oracle's tables initialise lazily: once, before the threads
    with cf.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        got = list(ex.map(lambda ki: gen.one(*ki), sample))
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import fs_chain_model
    bad = []
    for (k, idx), (dig, edge, (nb, i, j), rho) in zip(sample, got):
        pin, feat = oracle_pins.table(k)[idx], oracle_pins.features(k, idx)
        if dig != pin or edge != feat["alpha_edge"] or nb != feat["xof_blocks"]:
            bad.append((k, idx, dig != pin, edge, feat["alpha_edge"], nb, feat["xof_blocks"]))
        if nb > 3:
            assert fs_chain_model.gen_matrix_wave(rho, i, j, K=k)[1] == nb, (k, idx, i, j)
    assert len(sample) >= 39 and not bad, bad


def test_tape0_entries_agree_with_the_reference_digests():
    with open(os.path.join(ROOT, "tests", "golden", "kosk_tape_v1.json")) as f:
        gold = json.load(f)
    for k in (2, 3, 4):
        ref = gold["reference"][str(k)]
        pin = oracle_pins.table(k)[0]
        for f_, key in (("pk", "sha3_pk"), ("sk", "sha3_sk"), ("pi", "sha3_pi")):
            assert pin[f_] == bytes.fromhex(ref[key])[:len(pin[f_])], (k, f_)
        for idx in (0, 1):
            o = gold["oracle"]["k%d_tape%d" % (k, idx)]
            pin = oracle_pins.table(k)[idx]
            for f_, key in (("pk", "sha3_pk"), ("sk", "sha3_sk"), ("pi", "sha3_pi"), ("h1", "h1"), ("ch", "ch")):
                assert pin[f_] == bytes.fromhex(o[key])[:len(pin[f_])], (k, idx, f_)


def test_rare_features_occur_several_times_per_k():
    for k in (2, 3, 4):
        raw = oracle_pins._raw()["k%d" % k]
        assert len(raw["alpha_edge"]) >= MIN_RARE and len(raw["xof_blocks"]) >= MIN_RARE, (k, len(raw["alpha_edge"]), len(raw["xof_blocks"]))
        assert all(set(v) <= {0, 1, 3328} and v for v in raw["alpha_edge"].values())
        assert all(n >= 4 for n in raw["xof_blocks"].values())
        # the rare tapes land in the batches of the size sweeps (test_gpu_12), not only in the fixture
        from tests import test_gpu_12_batch_positions as t12
        s, w = t12.WINDOW[k]
        window = set(range(s, s + w))
        assert any(int(i) in window for i in raw["alpha_edge"]) and any(int(i) in window for i in raw["xof_blocks"]), k


def test_check_reports_every_mismatching_position():
    """swapped neighbours and a single changed secret key: every position that differs is reported, with the fields that differ"""
    k = 2
    with cf.ThreadPoolExecutor(3) as ex:
        out = list(ex.map(lambda i: oracle.verifiable_keygen(k, oracle.tape_bytes_for(k, i))[:3], range(3)))
    pks, sks, pis = (list(x) for x in zip(*out))
    assert oracle_pins.check(k, range(3), pks, sks, pis) == []
    sks[2] = sks[2][:-1] + bytes([sks[2][-1] ^ 1])
    assert oracle_pins.check(k, [1, 0, 2], pks, sks, pis) == [(0, 1, ["pk", "sk", "pi"]), (1, 0, ["pk", "sk", "pi"]), (2, 2, ["sk"])]
    assert oracle_pins.check(k, range(3), pis=pis[:2]) == [(None, None, ["pi: 2 outputs for 3 tapes"])]
