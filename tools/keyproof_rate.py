"""What proving for EXISTING keys costs next to proving with a key generation in front, Kyber-768, one handle (max_batch 736).

    python tools/keyproof_rate.py [--rounds 40] [--out profiles/keyproof_rate.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/keyproof_rate.py --kernels-only     (kernel times, a run of its own)

Step time, n = 46: stage_prover_keys + prove_resident next to stage_prover_inputs + prove_resident on the same 46 tapes (the keys of the
first are the ones the second generates), as ALTERNATING runs A B A B ... after a warm-up of both; host clock around calls that end
synchronised.  Reported per leg: median, quartiles, and the two halves of the step apart.  The spread that a difference has to
exceed is the quartile range of the same leg.
Witness call alone, n = 46 and n = 736: kosk_witness_from_sk on secret keys resident in HBM, se_out = NULL (D2D copy of the records,
launch_decode_pk's two launches, k_witness_from_sk, the ok bytes back), between two events on the handle's stream.
--kernels-only: just those witness calls (20 per size after a warm-up), for a kernel trace: k_witness_from_sk's own time is the
trace's figure, not this script's.
--summarise-trace DIR: no GPU; reads the *kernel_trace.csv files under DIR and prints, per kernel of a witness call and grid size,
the number of launches and the median / minimum duration.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, N, BIG = 3, 46, 736


def quart(xs):
    q = statistics.quantiles(xs, n=4)
    return "median %.1f us  quartiles %.1f .. %.1f  min %.1f" % (statistics.median(xs), q[0], q[2], min(xs))


def summarise_trace(root, say):
    import csv
    rows = {}
    for d, _, files in os.walk(root):
        for f in files:
            if not f.endswith("kernel_trace.csv"):
                continue
            with open(os.path.join(d, f), newline="") as fh:
                for r in csv.DictReader(fh):
                    r = {k.lower(): v for k, v in r.items()}
                    name = r.get("kernel_name", "")
                    if not any(x in name for x in ("k_witness_from_sk", "k_decode_pk", "k_gen_matrix_wave")):
                        continue
                    short = name.split("(")[0].split("::")[-1]
                    grid = int(r.get("grid_size_x", r.get("grid_size", "0")) or 0) * int(r.get("grid_size_y", "1") or 1)
                    wg = int(r.get("workgroup_size_x", "1") or 1)
                    rows.setdefault((short, grid // max(wg, 1)), []).append((int(r["end_timestamp"]) - int(r["start_timestamp"])) / 1e3)
    for (name, blocks), us in sorted(rows.items()):
        say("trace: %-20s %6d workgroups  %3d launches  median %.2f us  min %.2f us" % (name, blocks, len(us), statistics.median(us), min(us)))
    if not rows:
        say("trace: no launch of the witness call's kernels found under " + root)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=40)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--summarise-trace", metavar="DIR")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.summarise_trace:
        out = []
        summarise_trace(a.summarise_trace, lambda s: (print(s), out.append(s)))
        if a.out:
            with open(a.out, "a") as f:
                f.write("\n".join(out) + "\n")
        return
    import torch
    from mpcith_kyber_kosk_amd import api
    from tests import oracle_lib
    if not torch.cuda.is_available():
        raise SystemExit("tools/keyproof_rate.py needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ctx = api.Kosk(kyber_k=K, max_batch=BIG)
    tapes = [oracle_lib.tape_bytes_for(K, i, prefix="keyproof-rate:") for i in range(N)]
    ctx.stage_prover_inputs(tapes)
    sks = ctx.keys(N)[1]
    big = b"".join(sks[b % N] for b in range(BIG))
    d_sk = torch.frombuffer(bytearray(big), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()

    import ctypes as C
    lib, h, T = api.lib, ctx.handle, ctx.tape_bytes
    okbuf = C.create_string_buffer(BIG)
    skb, tpb = b"".join(sks), b"".join(t[:T] for t in tapes)
    pkout, skout = C.create_string_buffer(ctx.pk_bytes * N), C.create_string_buffer(ctx.sk_bytes * N)

    def must(rc, what):
        if rc:
            raise SystemExit(what + ": " + lib.kosk_last_error(h).decode())

    def witness_ms(n, calls):
        ctx.timer_start()
        for _ in range(calls):
            must(lib.kosk_witness_from_sk(h, n, C.c_void_p(d_sk.data_ptr()), None, okbuf), "kosk_witness_from_sk")
        ms = ctx.timer_stop_ms()
        assert okbuf.raw[:n] == b"\x01" * n
        return ms / calls

    for n in (N, BIG):
        witness_ms(n, 5)
    if a.kernels_only:
        for n in (N, BIG):
            witness_ms(n, 20)
        ctx.close()
        return
    say("keyproof_rate: Kyber-768, %s, one handle (max_batch %d), %d alternating rounds" % (torch.cuda.get_device_name(0), BIG, a.rounds))
    for n in (N, BIG):
        runs = [witness_ms(n, 20) * 1e3 for _ in range(5)]
        say("witness_from_sk alone, n %3d, sk resident in HBM, se_out NULL (copy + decode_pk + k_witness_from_sk + ok back): %s us per call, median %.1f"
            % (n, "  ".join("%.1f" % r for r in runs), statistics.median(runs)))

    def leg_keys():
        t0 = time.perf_counter()
        must(lib.kosk_stage_prover_keys(h, N, skb, tpb, T, okbuf), "kosk_stage_prover_keys")
        t1 = time.perf_counter()
        must(lib.kosk_prove_resident(h, N), "kosk_prove_resident")
        t2 = time.perf_counter()
        assert okbuf.raw[:N] == b"\x01" * N
        return (t1 - t0) * 1e6, (t2 - t1) * 1e6

    def leg_keygen():
        t0 = time.perf_counter()
        must(lib.kosk_stage_prover_inputs(h, N, tpb, T, pkout, skout), "kosk_stage_prover_inputs")
        t1 = time.perf_counter()
        must(lib.kosk_prove_resident(h, N), "kosk_prove_resident")
        t2 = time.perf_counter()
        return (t1 - t0) * 1e6, (t2 - t1) * 1e6
    for _ in range(5):
        leg_keys(); leg_keygen()
    leg_keygen()
    want = ctx.fetch_proofs(N)
    assert skout.raw == skb
    leg_keys()
    assert ctx.fetch_proofs(N) == want, "the two staging paths must give the same proofs"
    A, B = [], []
    for _ in range(a.rounds):
        A.append(leg_keys())
        B.append(leg_keygen())
    for name, runs in (("stage_prover_keys   + prove_resident", A), ("stage_prover_inputs + prove_resident", B)):
        say("%s, n %d: step   %s" % (name, N, quart([s + p for s, p in runs])))
        say("%s          staging %s" % (" " * len(name), quart([s for s, _ in runs])))
        say("%s          prove   %s" % (" " * len(name), quart([p for _, p in runs])))
    da = statistics.median(s + p for s, p in A) - statistics.median(s + p for s, p in B)
    say("difference of the step medians (existing keys - key generation): %+.1f us" % da)
    say("(host tapes and host sk records in pageable memory for both legs; the C entry points are called directly)")
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
