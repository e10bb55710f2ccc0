#!/usr/bin/env python3
"""Regenerates tests/golden/oracle_batch_pins_v1.json: what the CPU oracle (oracle/libkosk_oracle.so) returns for every
(Kyber K, tape index) that the GPU tests run in large batches, so that a test can check EVERY position of a batch, not a few.

Per tape "kosk-tape-v1:<index>" (tests/oracle_lib.py: tape_bytes_for) of ko_verifiable_keygen:
  pk, sk, pi   the first 8 bytes (64 bits) of SHA3-256 of the oracle's public key, secret key and proof image
  h1, ch       the first 4 bytes of the trace's h1 = SHA3-256(Tcomm[0..1454)) and ch = SHA3-256(view digests[0..1454)), i.e. of the
               two digest tables a resident batch keeps in HBM (kosk_resident_digests)
and two rare features of the tape's content, stored sparsely:
  alpha_edge   the tapes whose Fiat-Shamir challenges alpha[0 .. 70 + 2K) hold 0, 1 or q - 1 (the values those are)
  xof_blocks   the tapes for which some entry of gen_matrix(rho) needed more than three SHAKE128 blocks (how many, at most)
The digests of one K are concatenated in the order of its index ranges and stored base64-encoded.

Run from the repository root (takes a few minutes):  python tests/golden/make_oracle_pins.py
"""
import base64
import concurrent.futures as cf
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from tests import oracle_lib as o  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "oracle_batch_pins_v1.json")
Q = 3329
XOF_BLOCK = 168
DIGEST_BYTES = {"pk": 8, "sk": 8, "pi": 8, "h1": 4, "ch": 4}

# (first index, count) per Kyber K: every tape the GPU tests read in batches (the test that reads it in brackets)
RANGES = {
    2: [(0, 160),      # test_gpu_08 config 2 (0..45), test_gpu_12 size sweep and 46-proof verifier plan
        (5000, 72),    # gpu_child_cases.combined_calls (six callers x four rounds x three)
        (9500, 9)],    # gpu_child_cases.cohort_round_hooks
    3: [(0, 512),      # test_gpu_04 config 5, test_gpu_07 64-proof batch (100..163), test_gpu_12 sweeps, shapes, 64-proof plan
        (1000, 130),   # gpu_child_cases.big_batches
        (5000, 72),    # gpu_child_cases.combined_calls
        (7000, 7),     # gpu_child_cases.member_big_batch_stays_in_its_block: member 0
        (7100, 9),     #   and its neighbours
        (9000, 10),    # gpu_child_cases.combined_members_come_and_go
        (20000, 1472)],  # gpu_child_cases.line_of_record_shape: up to sixteen callers x two rounds (or six x three) x 46
    4: [(0, 2),        # the tapes kosk_tape_v1.json records
        (1000, 91),    # gpu_child_cases.big_batches
        (2000, 160),   # test_gpu_04 config 4 (2000..2090), test_gpu_12 size sweep
        (5000, 72)],   # gpu_child_cases.combined_calls
}


def xof_blocks(rho, i, j, nmax=8):
    """SHAKE128 blocks that rej_uniform reads before entry A[i][j] of gen_matrix(rho) has its 256 coefficients (indcpa.c:124-193;
    the stream is SHAKE128(rho || j || i), parsed in 3-byte groups, 56 per block)"""
    buf = hashlib.shake_128(bytes(rho) + bytes([j, i])).digest(XOF_BLOCK * nmax)
    ctr = 0
    for g in range(0, len(buf), 3):
        v0 = (buf[g] | (buf[g + 1] << 8)) & 0xFFF
        v1 = (buf[g + 1] >> 4) | (buf[g + 2] << 4)
        if v0 < Q:
            ctr += 1
        if ctr < 256 and v1 < Q:
            ctr += 1
        if ctr == 256:
            return g // XOF_BLOCK + 1
    raise AssertionError("more than %d blocks" % nmax)


def max_xof_blocks(k, pk):
    rho = pk[-32:]
    return max((xof_blocks(rho, i, j), i, j) for i in range(k) for j in range(k))


def one(k, idx):
    pk, sk, pi, _, _, tr = o.verifiable_keygen(k, o.tape_bytes_for(k, idx), trace=True)
    na = 70 + 2 * k
    edge = sorted({a for a in list(tr.alpha)[:na] if a in (0, 1, Q - 1)})
    d = {"pk": hashlib.sha3_256(pk).digest(), "sk": hashlib.sha3_256(sk).digest(), "pi": hashlib.sha3_256(pi).digest(),
         "h1": bytes(tr.h1), "ch": bytes(tr.ch)}
    return {f: d[f][:n] for f, n in DIGEST_BYTES.items()}, edge, max_xof_blocks(k, pk), pk[-32:]


def main():
    import fs_chain_model
    o.verifiable_keygen(2, o.tape_bytes_for(2, 0))  # the oracle's tables initialise lazily: once, before the threads start
    out = {"about": "tests/golden/make_oracle_pins.py: oracle digests of ko_verifiable_keygen per (K, tape index)",
           "tape_seed_format": "kosk-tape-v1:<index>", "digest_bytes": DIGEST_BYTES}
    threads = min(16, os.cpu_count() or 1)
    checked = 0
    with cf.ThreadPoolExecutor(threads) as pool:
        for k in (2, 3, 4):
            idxs = [s + i for s, c in RANGES[k] for i in range(c)]
            res = list(pool.map(lambda i: one(k, i), idxs))
            ent = {"ranges": [list(r) for r in RANGES[k]], "alpha_edge": {}, "xof_blocks": {}}
            for f in DIGEST_BYTES:
                ent[f] = base64.b64encode(b"".join(r[0][f] for r in res)).decode()
            for idx, (_, edge, (nb, i, j), rho) in zip(idxs, res):
                if edge:
                    ent["alpha_edge"][str(idx)] = edge
                if nb > 3:
                    ent["xof_blocks"][str(idx)] = nb
                    if checked < 24:  # the block count against the lane-level model of the kernel's wave sponge
                        assert fs_chain_model.gen_matrix_wave(rho, i, j, K=k)[1] == nb, (k, idx, i, j)
                        checked += 1
            out["k%d" % k] = ent
            print("K=%d: %d tapes, %d with an alpha edge value, %d with more than three XOF blocks" %
                  (k, len(idxs), len(ent["alpha_edge"]), len(ent["xof_blocks"])))
    assert checked > 0
    with open(OUT, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", os.path.relpath(OUT, ROOT), os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
