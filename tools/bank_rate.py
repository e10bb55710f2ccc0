"""What the offline bank takes off a prove-keys step, Kyber-768, one handle (max_batch 736, bank capacity 736), n = 1, 46 and 736.

    python tools/bank_rate.py [--parent-lib PATH] [--rounds 30] [--out profiles/bank_rate.txt]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bank_rate.py --kernels-only     (kernel times, a run of its own)
    python tools/bank_rate.py --summarise-trace DIR [--out FILE]                                                (no GPU)

Steps, as ALTERNATING rounds a b d c a b d c ... after a warm-up of all, host clock around calls that end synchronised, the C entry
points called directly, host tapes and sk records in pageable memory for every leg:
  (a) kosk_stage_prover_keys + kosk_prove_resident on the parent commit's library (--parent-lib: another build of this library, loaded
      beside this tree's; without it the leg is left out)
  (b) the same on this tree
  (c) kosk_stage_prover_keys_banked + kosk_prove_resident
  (d) kosk_bank_fill of the n entries that (c) consumes, per entry
Reported per leg: median, quartiles, minimum; the spread a difference has to exceed is the quartile range of the same leg.
Kernel yardstick: kosk_bank_timing -- k_bank_put and k_bank_take of n entries between two events, next to the runtime's own two strided
hipMemcpy2DAsync D2D copies of the same bytes and those copies plus its hipMemsetAsync of the slots.  --kernels-only runs just that, for
a kernel trace; --summarise-trace prints the two kernels' durations per grid size from the trace.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, SIZES, BIG = 3, (1, 46, 736), 736


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
                    if "k_bank_" not in name:
                        continue
                    short = name.split("(")[0].split("::")[-1]
                    wgs = 1
                    for ax in "xyz":
                        g, w = int(r.get("grid_size_" + ax, "1") or 1), int(r.get("workgroup_size_" + ax, "1") or 1)
                        wgs *= max(g // max(w, 1), 1)
                    rows.setdefault((short, wgs), []).append((int(r["end_timestamp"]) - int(r["start_timestamp"])) / 1e3)
    for (name, blocks), us in sorted(rows.items()):
        say("trace: %-12s %6d workgroups  %3d launches  median %.2f us  min %.2f us" % (name, blocks, len(us), statistics.median(us), min(us)))
    if not rows:
        say("trace: no launch of k_bank_put / k_bank_take found under " + root)


def parent_handle(path):
    """the five calls leg (a) needs, on another build of the library"""
    lib = C.CDLL(path)
    vp, sz = C.c_void_p, C.c_size_t
    lib.kosk_create.restype, lib.kosk_create.argtypes = C.c_int, [C.POINTER(vp), C.c_int, C.c_int, C.c_int]
    lib.kosk_destroy.restype, lib.kosk_destroy.argtypes = None, [vp]
    lib.kosk_last_error.restype, lib.kosk_last_error.argtypes = C.c_char_p, [vp]
    lib.kosk_stage_prover_keys.restype, lib.kosk_stage_prover_keys.argtypes = C.c_int, [vp, C.c_int, vp, vp, sz, vp]
    lib.kosk_prove_resident.restype, lib.kosk_prove_resident.argtypes = C.c_int, [vp, C.c_int]
    lib.kosk_fetch_proofs.restype, lib.kosk_fetch_proofs.argtypes = C.c_int, [vp, C.c_int, vp]
    h = vp()
    if lib.kosk_create(C.byref(h), 0, K, BIG):
        raise SystemExit("kosk_create on the parent library failed")
    return lib, h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--summarise-trace", metavar="DIR")
    ap.add_argument("--out")
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def finish(mode):
        if a.out:
            with open(a.out, mode) as f:
                f.write("\n".join(lines) + "\n")
    if a.summarise_trace:
        summarise_trace(a.summarise_trace, say)
        return finish("a")
    import torch
    from mpcith_kyber_kosk_amd import api
    from tests import oracle_lib
    if not torch.cuda.is_available():
        raise SystemExit("tools/bank_rate.py needs a GPU")
    ctx = api.Kosk(kyber_k=K, max_batch=BIG)
    ctx.bank_reserve(BIG)
    if a.kernels_only:
        for n in SIZES:
            ctx.bank_timing(n, reps=20)
        ctx.close()
        return
    lib, h, T = api.lib, ctx.handle, ctx.tape_bytes
    base = [oracle_lib.tape_bytes_for(K, i, prefix="bank-rate:") for i in range(46)]
    ctx.stage_prover_inputs(base)
    sks = ctx.keys(46)[1]
    skb = b"".join(sks[b % 46] for b in range(BIG))
    tpb = b"".join(base[b % 46][:T] for b in range(BIG))
    okbuf = C.create_string_buffer(BIG)
    plib, ph = parent_handle(a.parent_lib) if a.parent_lib else (None, None)

    def must(rc, what, L=lib, H=h):
        if rc:
            raise SystemExit(what + ": " + L.kosk_last_error(H).decode())

    def leg_plain(L, H, n):
        t0 = time.perf_counter()
        must(L.kosk_stage_prover_keys(H, n, skb, tpb, T, okbuf), "kosk_stage_prover_keys", L, H)
        t1 = time.perf_counter()
        must(L.kosk_prove_resident(H, n), "kosk_prove_resident", L, H)
        t2 = time.perf_counter()
        return (t1 - t0) * 1e6, (t2 - t1) * 1e6

    def leg_fill(n):
        t0 = time.perf_counter()
        must(lib.kosk_bank_fill(h, n, tpb, T, None, 0), "kosk_bank_fill")
        return (time.perf_counter() - t0) * 1e6

    def leg_banked(n):
        t0 = time.perf_counter()
        must(lib.kosk_stage_prover_keys_banked(h, n, skb, tpb, T, None, 0, okbuf), "kosk_stage_prover_keys_banked")
        t1 = time.perf_counter()
        must(lib.kosk_prove_resident(h, n), "kosk_prove_resident")
        t2 = time.perf_counter()
        return (t1 - t0) * 1e6, (t2 - t1) * 1e6

    say("bank_rate: Kyber-768, %s, one handle (max_batch %d, bank capacity %d), alternating rounds" % (torch.cuda.get_device_name(0), BIG, BIG))
    say("entry: %d bytes" % api.bank_entry_bytes(K))
    for n in SIZES:
        rounds = a.rounds if n < BIG else max(a.rounds // 3, 5)
        for _ in range(3):
            if plib:
                leg_plain(plib, ph, n)
            leg_plain(lib, h, n); leg_fill(n); leg_banked(n)
        leg_plain(lib, h, n)
        want = ctx.fetch_proofs(n)
        leg_fill(n); leg_banked(n)
        assert ctx.fetch_proofs(n) == want, "the banked step must give the same proofs on the same tapes"
        if plib:
            leg_plain(plib, ph, n)
            buf = C.create_string_buffer(ctx.proof_bytes * n)
            must(plib.kosk_fetch_proofs(ph, n, buf), "kosk_fetch_proofs", plib, ph)
            assert buf.raw == b"".join(want), "the parent library must give the same proofs"
        A, B, Cc, D = [], [], [], []
        for _ in range(rounds):
            if plib:
                A.append(leg_plain(plib, ph, n))
            B.append(leg_plain(lib, h, n))
            D.append(leg_fill(n))
            Cc.append(leg_banked(n))
        say("n %d, %d rounds" % (n, rounds))
        for name, runs in (("(a) parent: stage_prover_keys + prove_resident       ", A), ("(b) this tree: stage_prover_keys + prove_resident    ", B),
                           ("(c) stage_prover_keys_banked + prove_resident       ", Cc)):
            if not runs:
                continue
            say("  %s step    %s" % (name, quart([s + p for s, p in runs])))
            say("  %s staging %s" % (" " * len(name), quart([s for s, _ in runs])))
            say("  %s prove   %s" % (" " * len(name), quart([p for _, p in runs])))
        say("  (d) kosk_bank_fill of %d entries                       call    %s" % (n, quart(D)))
        say("  %s per entry %.1f us" % (" " * 53, statistics.median(D) / n))
        mb, mc = statistics.median(s + p for s, p in B), statistics.median(s + p for s, p in Cc)
        if A:
            ma = statistics.median(s + p for s, p in A)
            say("  step medians: (b) - (a) %+.1f us;  (c) - (a) %+.1f us = %+.1f %%" % (mb - ma, mc - ma, 100 * (mc - ma) / ma))
        say("  step medians: (c) - (b) %+.1f us = %+.1f %%" % (mc - mb, 100 * (mc - mb) / mb))
    if plib:
        plib.kosk_destroy(ph)
    say("kernel yardstick (kosk_bank_timing, 20 launches between two events each; copy = the runtime's two strided D2D copies of the same bytes, fill = its memset of the slots):")
    for n in SIZES:
        t = ctx.bank_timing(n, reps=20)
        gb = lambda ms, passes: passes * t["bytes"] / (ms * 1e-3) / 1e9  # noqa: E731
        say("  n %3d, %9d bytes: k_bank_put %.2f us (%.0f GB/s read + written)  k_bank_take %.2f us (%.0f GB/s read + written + zeroed)  "
            "copy %.2f us  copy + fill %.2f us  take / (copy + fill) %.2f"
            % (n, t["bytes"], t["put_ms"] * 1e3, gb(t["put_ms"], 2), t["take_ms"] * 1e3, gb(t["take_ms"], 3), t["copy_ms"] * 1e3,
               t["copy_fill_ms"] * 1e3, t["take_ms"] / t["copy_fill_ms"]))
    ctx.close()
    finish("w")


if __name__ == "__main__":
    main()
