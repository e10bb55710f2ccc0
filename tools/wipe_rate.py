"""What erasing secrets costs (k_wipe), Kyber-768, one handle, n = 46 proofs per call.

    python tools/wipe_rate.py [--rounds 5] [--calls 10] [--reps 20] [--parent-lib PATH] [--out profiles/wipe_rate.txt]

k_wipe alone: kosk_wipe_timing on handles of max_batch 46, 184, 300 and 736 (the row matrix, the largest single run, is about 300 MiB at 184: the last size at which k_wipe clears it) -- the bytes one wipe clears in HBM (the secret
regions of the inventory, per proof), `reps` wipes of them as the library issues them (one launch of k_wipe; a single run of 320 MiB or
more goes to the runtime's fill instead) between two events on the handle's stream, and, as the yardstick,
`reps` rounds of the runtime's own fills of the same regions (one hipMemsetAsync per region) between two events on the same stream;
`rounds` repeats, reported: every repeat and the median.
The mode: proofs/s of kosk_prove_keys_batch and of kosk_verifiable_keygen_resident + kosk_verify_resident_pk (host tapes, wall clock
around calls that end synchronised) with KOSK_WIPE_CALL against KOSK_WIPE_OFF on two handles of this library, as ALTERNATING legs
after a warm-up of both, `calls` calls per leg and round; the cost is the ratio of the medians, the spread the lowest and highest
round over the median.
Mode off against the parent commit's library (--parent-lib, through KOSK_LIB_PATH in a child process, alternating with child
processes on this library): the same two workloads; the difference of the medians has to lie within the spread of the rounds.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, N, SIZES = 3, 46, (46, 184, 300, 736)


def workloads(api, ctx):
    from tests import oracle_lib
    tapes = [oracle_lib.tape_bytes_for(K, b, prefix="wipe-rate:") for b in range(N)]
    sks = [api.host_keygen(K, oracle_lib.tape_bytes_for(K, b, prefix="wipe-rate:key:")[:64])[1] for b in range(N)]

    def prove_keys():
        _pis, ok = ctx.prove_keys(sks, tapes=tapes)
        assert all(ok)

    def keygen_verify():
        ctx.verifiable_keygen_resident(tapes)
        assert ctx.verify_resident_pk(N) == [True] * N
    return (("prove_keys", prove_keys), ("keygen + verify", keygen_verify))


def leg(fn, calls):
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    return calls * N / (time.perf_counter() - t0)


def off_leg(rounds, calls):
    """in THIS process (the library is whatever KOSK_LIB_PATH names), mode off: proofs/s per workload and round, one JSON line"""
    from mpcith_kyber_kosk_amd import api
    ctx = api.Kosk(kyber_k=K, max_batch=N)
    out = {}
    for name, fn in workloads(api, ctx):
        leg(fn, 3)
        out[name] = [leg(fn, calls) for _ in range(rounds)]
    ctx.close()
    print(json.dumps(out), flush=True)


def spread(v):
    m = statistics.median(v)
    return m, min(v) / m, max(v) / m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-lib", default="", help="the parent commit's libkosk_mi355x.so (without it that comparison is left out)")
    ap.add_argument("--out")
    ap.add_argument("--off-leg", action="store_true", help="(internal) run the mode-off legs in this process")
    a = ap.parse_args()
    if a.off_leg:
        off_leg(a.rounds, a.calls)
        return
    import torch
    from mpcith_kyber_kosk_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("tools/wipe_rate.py needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("wipe_rate: Kyber-768, %s, %d proofs per call, %d rounds" % (torch.cuda.get_device_name(0), N, a.rounds))
    for mb in SIZES:
        ctx = api.Kosk(kyber_k=K, max_batch=mb)
        ctx.wipe_timing(3)
        runs = [ctx.wipe_timing(a.reps) for _ in range(a.rounds)]
        nbytes, regions = runs[0][2], runs[0][3]
        w, m = statistics.median(r[0] for r in runs) * 1e3, statistics.median(r[1] for r in runs) * 1e3
        say("max_batch %3d: one wipe clears %d bytes of HBM in %d regions = %d bytes per proof" % (mb, nbytes, regions, nbytes // mb))
        say("  the wipe (k_wipe + fill)  : %s us, median %.1f us = %.2f TB/s" % ("  ".join("%.1f" % (r[0] * 1e3) for r in runs), w, nbytes / w / 1e6))
        say("  hipMemsetAsync per region : %s us, median %.1f us = %.2f TB/s" % ("  ".join("%.1f" % (r[1] * 1e3) for r in runs), m, nbytes / m / 1e6))
        say("  the wipe / memsets        : %.3f" % (w / m))
        ctx.close()
    on, off = api.Kosk(kyber_k=K, max_batch=N), api.Kosk(kyber_k=K, max_batch=N)
    on.set_wipe(api.WIPE_CALL)
    for (name, f_on), (_n, f_off) in zip(workloads(api, on), workloads(api, off)):
        for _ in range(2):
            leg(f_on, 2); leg(f_off, 2)
        A, B = [], []
        for _ in range(a.rounds):
            A.append(leg(f_on, a.calls))
            B.append(leg(f_off, a.calls))
        (ma, la, ha), (mb_, lb, hb) = spread(A), spread(B)
        say("%-15s KOSK_WIPE_CALL: %s proofs/s, median %.0f (rounds %.3f .. %.3f of it)" % (name, "  ".join("%.0f" % x for x in A), ma, la, ha))
        say("%-15s KOSK_WIPE_OFF : %s proofs/s, median %.0f (rounds %.3f .. %.3f of it)" % (name, "  ".join("%.0f" % x for x in B), mb_, lb, hb))
        say("%-15s on / off      : %.3f (%.1f us per call of %d proofs)" % (name, ma / mb_, (1 / ma - 1 / mb_) * N * 1e6, N))
    say("launches of k_wipe on the handle in KOSK_WIPE_CALL: %d; on the other: %d" % (on.path_count(api.Kosk.PATH_WIPE), off.path_count(api.Kosk.PATH_WIPE)))
    on.close(); off.close()
    if not a.parent_lib:
        say("(no --parent-lib: mode off against the parent commit's library is left out)")
    else:
        res = {"this": {}, "parent": {}}
        for rnd in range(2):  # child processes, alternating: this library, the parent's, this, the parent's
            for who in ("this", "parent"):
                env = dict(os.environ)
                if who == "parent":
                    env["KOSK_LIB_PATH"] = os.path.abspath(a.parent_lib)
                else:
                    env.pop("KOSK_LIB_PATH", None)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--off-leg", "--rounds", str(a.rounds), "--calls", str(a.calls)],
                                   cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
                if r.returncode:
                    raise SystemExit("the mode-off leg failed (exit %d)\n%s" % (r.returncode, r.stderr[-2000:]))
                for name, v in json.loads(r.stdout.strip().splitlines()[-1]).items():
                    res[who].setdefault(name, []).extend(v)
        for name in res["this"]:
            (mt, lt, ht), (mp, lp, hp) = spread(res["this"][name]), spread(res["parent"][name])
            say("%-15s mode off, this library  : %s proofs/s, median %.0f (rounds %.3f .. %.3f of it)" % (name, "  ".join("%.0f" % x for x in res["this"][name]), mt, lt, ht))
            say("%-15s parent commit's library : %s proofs/s, median %.0f (rounds %.3f .. %.3f of it)" % (name, "  ".join("%.0f" % x for x in res["parent"][name]), mp, lp, hp))
            inside = min(lt, lp) <= mt / mp <= max(ht, hp)
            say("%-15s this / parent           : %.3f -- %s the run-to-run spread of the rounds" % (name, mt / mp, "within" if inside else "OUTSIDE"))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
