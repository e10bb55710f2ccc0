"""What seeded proving buys: the throughput of bench.py's arrangement with the randomness of every proof coming from five sources.

    python tools/seeded_rate.py [--parent-lib PATH/libkosk_mi355x.so] [--seconds 2] [--repeats 3] [--shapes host,device] [--out FILE]
    python tools/seeded_rate.py --leg B --shape host [--short]        # ONE leg in this process (what the driver spawns; for profilers)

Shapes: `host` = the line of record (K = 3, 46 proofs per call, 18 caller threads, cohorts of 6, host Fiat-Shamir), `device` = 48
callers in cohorts of 16 with the Fiat-Shamir rounds on the device.  A step is what bench.py times: kosk_verifiable_keygen_resident
(key generation + prove) and kosk_verify_resident_pk, every verify bit asserted.  Legs:

    A0  resident device tape banks (bench.py's shape), on ANOTHER build of the library (--parent-lib, loaded through KOSK_LIB_PATH)
    A1  the same on this tree
    B   kosk_verifiable_keygen_seeded_resident with fresh host seeds every call (32 bytes per proof cross PCIe)
    C   tapes = NULL in the default mode: the library draws 68 KB per proof from OS entropy in the reference's call sequence
    D   tapes = NULL after kosk_set_entropy(KOSK_ENTROPY_SEED): one 32-byte draw per proof

Every leg runs in a fresh child process (one library per process), warms up, then counts the steps completed inside a window of
--seconds.  The legs alternate --repeats times in one command; medians and the spread of A0 are printed at the end.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"host": dict(callers=18, combine=6, fs="host"), "device": dict(callers=48, combine=16, fs="device")}
LEGS = ["A0", "A1", "B", "C", "D"]
K, BATCH, TAPE_SETS = 3, 46, 4


def run_leg(leg, shape, seconds, warm):
    import torch
    import bench
    from mpcith_kyber_kosk_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("tools/seeded_rate.py needs a GPU")
    sh = SHAPES[shape]
    S, CMB = sh["callers"], sh["combine"]
    cores = bench.usable_host_cores()
    threads, blocking = bench.host_budget(cores, 1, -(-S // CMB), bench.CONFIGS[3]["threads"] * CMB)
    threads = 1 if sh["fs"] == "device" else bench.threads_per_caller(threads, blocking, CMB, cores)
    slots = [bench.Slot(api, torch, K, BATCH, 0, si * TAPE_SETS * BATCH, TAPE_SETS, combine=CMB, fs=sh["fs"], threads=threads, blocking=blocking)
             for si in range(S)]
    lib = api.lib
    ones = b"\x01" * BATCH

    def make_step(sl):
        if leg in ("A0", "A1"):
            return lambda i: sl.step(torch, i)
        h = sl.c.handle
        pk = C.create_string_buffer(sl.c.pk_bytes * BATCH); sk = C.create_string_buffer(sl.c.sk_bytes * BATCH)
        ok = C.create_string_buffer(BATCH)
        if leg == "D":
            sl.c.set_entropy(api.ENTROPY_SEED)
        if leg == "B":
            seeded = lib.kosk_verifiable_keygen_seeded_resident

            def keygen(i):
                return seeded(h, BATCH, os.urandom(32 * BATCH), 32, pk, sk)  # fresh host seeds every call
        else:
            def keygen(i):
                return lib.kosk_verifiable_keygen_resident(h, BATCH, None, 0, pk, sk)

        def step(i):
            if keygen(i):
                sl.c._chk(1, "keygen")
            if lib.kosk_verify_resident_pk(h, BATCH, None, ok):
                sl.c._chk(1, "verify_resident_pk")
            if ok.raw != ones:
                raise RuntimeError("the verifier rejected an honest proof")
        return step
    steps = [make_step(sl) for sl in slots]
    for st in steps:
        st(0)  # setup: first use allocates the verifier's workspace
    done, errs = [], []
    stop = threading.Event()

    def worker(si):
        try:
            i = si
            while not stop.is_set():
                steps[si](i)
                done.append(time.perf_counter())
                i += S
        except Exception as e:  # noqa: BLE001
            errs.append(repr(e))
            stop.set()
    import gc
    gc.collect()
    gc.freeze()
    gc.disable()
    ths = [threading.Thread(target=worker, args=(si,), daemon=True) for si in range(S)]
    t_start = time.perf_counter()
    for t in ths:
        t.start()
    time.sleep(warm)
    t0 = time.perf_counter()
    time.sleep(seconds)
    t1 = time.perf_counter()
    stop.set()
    for t in ths:
        t.join()
    torch.cuda.synchronize()
    if errs:
        raise SystemExit("leg %s failed: %s" % (leg, errs[0]))
    n = sum(1 for x in done if t0 <= x < t1)
    calls = members = 0
    for sl in slots:
        a, b = sl.c.combine_stats()
        calls += a; members += b
    pc = {}
    if hasattr(lib, "kosk_tape_from_seed"):  # (an older build on leg A0 does not know the newest path id)
        for sl in slots:
            for name, v in sl.c.path_counts().items():
                pc[name] = pc.get(name, 0) + v
    out = {"leg": leg, "shape": shape, "library": os.path.relpath(api.LIB_PATH, ROOT), "callers": S, "handles_per_cohort": CMB, "fiat_shamir": sh["fs"],
           "host_threads_per_caller": threads, "window_s": round(t1 - t0, 4), "warm_s": round(t0 - t_start, 3), "steps_in_window": n,
           "proofs_per_s": round(n * BATCH / (t1 - t0), 1), "mean_callers_per_run": round(members / calls, 2) if calls else 0.0,
           "tape_expand_launches": pc.get("tape_expand", 0), "small_copy_kernel": pc.get("small_copy_kernel", 0)}
    for sl in slots:
        sl.c.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", default="", choices=[""] + LEGS)
    ap.add_argument("--shape", default="host", choices=sorted(SHAPES))
    ap.add_argument("--shapes", default="host,device")
    ap.add_argument("--seconds", type=float, default=2.0, help="timed window per leg (after the warm-up)")
    ap.add_argument("--warm", type=float, default=1.0)
    ap.add_argument("--short", action="store_true", help="with --leg: 0.5 s warm-up and a 1 s window (profiler runs)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-lib", default="", help="the build leg A0 runs on (a libkosk_mi355x.so of the parent commit)")
    ap.add_argument("--out", default="", help="also write the report to this file")
    args = ap.parse_args()
    if args.leg:
        if args.short:
            args.warm, args.seconds = 0.5, 1.0
        sys.stdout.flush()
        fd = os.dup(1)
        os.dup2(2, 1)  # stdout carries one JSON line
        res = run_leg(args.leg, args.shape, args.seconds, args.warm)
        os.write(fd, (json.dumps(res) + "\n").encode())
        return
    legs = [l for l in LEGS if l != "A0" or args.parent_lib]
    if args.out:
        open(args.out, "w").close()

    def say(s):
        print(s, flush=True)
        if args.out:  # line by line: a run that ends early leaves what it measured
            with open(args.out, "a") as f:
                f.write(s + "\n")
    say("# tools/seeded_rate.py: K = %d, %d proofs per call, window %.1f s after %.1f s warm-up, legs alternated %d times" % (K, BATCH, args.seconds, args.warm, args.repeats))
    for shape in args.shapes.split(","):
        rates = {l: [] for l in legs}
        for rep in range(args.repeats):
            for leg in legs:
                env = dict(os.environ)
                env.pop("KOSK_LIB_PATH", None)
                if leg == "A0":
                    env["KOSK_LIB_PATH"] = os.path.abspath(args.parent_lib)
                cmd = [sys.executable, os.path.abspath(__file__), "--leg", leg, "--shape", shape, "--seconds", str(args.seconds), "--warm", str(args.warm)]
                r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
                if r.returncode != 0:
                    say("leg %s shape %s repeat %d FAILED (exit %d): %s" % (leg, shape, rep, r.returncode, r.stderr[-1500:]))
                    raise SystemExit(1)  # nothing more is started after a failed GPU step
                res = json.loads(r.stdout.strip().splitlines()[-1])
                rates[leg].append(res["proofs_per_s"])
                say(json.dumps(res))
        say("## shape %s: medians (proofs/s)" % shape)
        med = {l: statistics.median(v) for l, v in rates.items()}
        for l in legs:
            say("  %-2s median %10.1f   runs %s" % (l, med[l], " ".join("%.1f" % x for x in rates[l])))
        if "A0" in med:
            a0 = rates["A0"]
            say("  A0 spread over its repeats: %.1f .. %.1f (%.2f %% of the median)" % (min(a0), max(a0), 100.0 * (max(a0) - min(a0)) / med["A0"]))
            say("  A1 / A0 = %.4f   B / A0 = %.4f (wanted >= 0.95)   D / A0 = %.4f   C / A0 = %.4f" % (med["A1"] / med["A0"], med["B"] / med["A0"], med["D"] / med["A0"], med["C"] / med["A0"]))
        say("  per caller thread: C %.1f proofs/s, D %.1f proofs/s" % (med["C"] / SHAPES[shape]["callers"], med["D"] / SHAPES[shape]["callers"]))


if __name__ == "__main__":
    main()
