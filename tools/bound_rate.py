"""What binding costs: proofs/s of an ARMED handle (kosk_set_contexts, format kosk-bind-v1) next to an unarmed one and next to the parent
commit's library, at bench.py's line-of-record call shape (Kyber-768, 46 proofs per call), in both Fiat-Shamir modes.

    python tools/bound_rate.py [--parent-lib PATH] [--rounds 6] [--calls 150] [--out profiles/bound_rate.txt]

One step = kosk_verifiable_keygen_resident + kosk_verify_resident_pk(pk == NULL) on ONE uncombined handle of 46 (an armed handle keeps
its calls out of merged runs, INTEGRATION.md 10: the cohort arrangement of the benchmark is not what an armed caller gets), device tapes
read in place, host clock around `calls` steps that each end synchronised.  Legs, per Fiat-Shamir mode:
    parent    the parent commit's library through KOSK_LIB_PATH (the A/B rule of mpcith_kyber_kosk_amd/api.py), unarmed; a child process
    unarmed   this tree's library, never armed
    armed     this tree's library, armed with 46 contexts
run as ALTERNATING rounds  parent, unarmed, armed, parent, unarmed, armed, ...  (every leg a fresh child process, so that all three start
from the same state; a warm-up of 30 steps in each).  Reported per leg: the rounds' rates, their median, minimum and maximum.  The spread
a difference has to exceed is the min-max range of the same leg.  No threshold is asserted: the expectation from the permutation count
(one more small launch per call, no more Keccak permutations in the chains) had not been measured before this tool.
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
K, N = 3, 46


def leg(fs, armed, calls):
    """one leg in THIS process: steps per second -> proofs/s, printed as one JSON line"""
    import hashlib
    import torch
    from mpcith_kyber_kosk_amd import api
    from tests import oracle_lib
    ctx = api.Kosk(kyber_k=K, max_batch=N, fs_mode=api.FS_DEVICE if fs == "device" else api.FS_HOST)
    T = ctx.tape_bytes
    stride = (T + 63) // 64 * 64
    blob = bytearray(stride * N)
    for b in range(N):
        blob[b * stride:b * stride + T] = oracle_lib.tape_bytes_for(K, b, prefix="bound-rate:")
    d_tapes = torch.frombuffer(blob, dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    if armed:
        ctx.set_contexts([hashlib.sha3_256(b"bound-rate-context:%d" % b).digest() for b in range(N)])

    def step():
        ctx.verifiable_keygen_resident(d_tapes.data_ptr(), n=N, tape_stride=stride)
        return ctx.verify_resident_pk(N)
    for _ in range(30):
        bits = step()
    assert bits == [True] * N
    t0 = time.perf_counter()
    for _ in range(calls):
        step()
    dt = time.perf_counter() - t0
    ctx.close()
    print(json.dumps({"fs": fs, "armed": bool(armed), "proofs_per_s": calls * N / dt, "step_us": dt / calls * 1e6}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="the parent commit's libkosk_mi355x.so (without it the parent leg is left out)")
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--calls", type=int, default=150)
    ap.add_argument("--out")
    ap.add_argument("--leg", default="", help="(internal) fs:armed -- run one leg in this process")
    a = ap.parse_args()
    if a.leg:
        fs, armed = a.leg.split(":")
        leg(fs, armed == "1", a.calls)
        return
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("tools/bound_rate.py needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def child(fs, armed, lib):
        env = dict(os.environ)
        env.pop("KOSK_LIB_PATH", None)
        if lib:
            env["KOSK_LIB_PATH"] = lib
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "%s:%d" % (fs, armed), "--calls", str(a.calls)], cwd=ROOT, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
        if r.returncode:
            raise SystemExit("leg %s armed=%d lib=%s failed (exit %d)\n%s" % (fs, armed, lib or "tree", r.returncode, r.stderr[-2000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])["proofs_per_s"]
    say("bound_rate: Kyber-768, %d proofs per call, one uncombined handle, %s; %d alternating rounds of %d steps (keygen_resident + verify_resident_pk)"
        % (N, torch.cuda.get_device_name(0), a.rounds, a.calls))
    if not a.parent_lib:
        say("(no --parent-lib: the parent leg is left out)")
    for fs in ("host", "device"):
        legs = ([("parent, unarmed", 0, a.parent_lib)] if a.parent_lib else []) + [("this tree, unarmed", 0, ""), ("this tree, armed", 1, "")]
        rates = {name: [] for name, _, _ in legs}
        for _ in range(a.rounds):
            for name, armed, lib in legs:
                rates[name].append(child(fs, armed, lib))
        for name, _, _ in legs:
            xs = rates[name]
            say("fs %-6s %-20s proofs/s: %s   median %.0f  min %.0f  max %.0f" % (fs, name, " ".join("%.0f" % x for x in xs), statistics.median(xs), min(xs), max(xs)))
        un, ar = statistics.median(rates["this tree, unarmed"]), statistics.median(rates["this tree, armed"])
        say("fs %-6s armed / unarmed (medians): %.4f   step %.1f us -> %.1f us" % (fs, ar / un, N / un * 1e6, N / ar * 1e6))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
