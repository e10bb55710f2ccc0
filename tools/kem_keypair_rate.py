"""Key pairs per second of kosk_kem_keypair_batch, Kyber-768, next to what else makes or uses keys on the same box in the same run.

    python tools/kem_keypair_rate.py [--sizes 46,4096,65536] [--seconds 1.0] [--repeats 3] [--parent-lib PATH] [--out profiles/kem_keypair_rate.txt]

Per n: coins and both outputs resident in HBM (torch tensors handed over as device pointers); each shape is warmed up, then whole calls
are counted inside a window of at least --seconds between two events on the handle's stream (kosk_stream_timer_start / _stop; every
call ends synchronised, so the window holds complete calls only), --repeats times.  n = 4096 is also run with host buffers.  The keys of
the first call of each shape pass kosk_kem_check_sk, and the checks are timed the same way.  Next to it:
    kem_enc    kosk_kem_enc_batch at the same n, device buffers, to the keys just made: about the same hash and NTT work per item
    reference  pqcrystals_kyber768_ref_keypair_derand (kyber/kem.c, compiled into oracle/_ref by oracle/Makefile) through ctypes on one
               core; skipped with a note where oracle/_ref is absent
    prover     kosk_stage_prover_inputs at max_batch = 46 with host tapes on the parent commit's library (--parent-lib, through
               KOSK_LIB_PATH in a child process): how key pairs left the GPU before this call existed; left out without --parent-lib
No rate is asserted: none had been measured before this tool.
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, PROVER_BATCH = 3, 46


def window(ctx, call, n, seconds):
    """items/s over whole calls inside >= `seconds`, by the stream events; (rate by events, rate by wall clock, calls)"""
    calls = 0
    ctx.timer_start()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        call()
        calls += 1
    wall = time.perf_counter() - t0
    ms = ctx.timer_stop_ms()
    return n * calls / (ms * 1e-3), n * calls / wall, calls


def reference_rate(seconds):
    path = os.path.join(ROOT, "oracle", "_ref", "libkyber_ref_k%d.so" % K)
    if not os.path.exists(path):
        return None
    fn = C.CDLL(path).pqcrystals_kyber768_ref_keypair_derand
    pk, sk = C.create_string_buffer(1184), C.create_string_buffer(2400)
    coins = hashlib.shake_256(b"keypair-rate").digest(64)
    for _ in range(200):
        fn(pk, sk, coins)
    n, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        for _ in range(100):
            fn(pk, sk, coins)
        n += 100
    return n / (time.perf_counter() - t0)


def prover_leg(seconds):
    """in THIS process (the library is whatever KOSK_LIB_PATH names): key pairs/s of kosk_stage_prover_inputs, one JSON line"""
    from mpcith_kyber_kosk_amd import api
    from tests import oracle_lib
    ctx = api.Kosk(kyber_k=K, max_batch=PROVER_BATCH)
    tapes = [oracle_lib.tape_bytes_for(K, b, prefix="keypair-rate:") for b in range(PROVER_BATCH)]
    for _ in range(5):
        ctx.stage_prover_inputs(tapes)
    calls, t0 = 0, time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        ctx.stage_prover_inputs(tapes)
        calls += 1
    dt = time.perf_counter() - t0
    ctx.close()
    print(json.dumps({"keypairs_per_s": calls * PROVER_BATCH / dt, "calls": calls}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="46,4096,65536")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-lib", default="", help="the parent commit's libkosk_mi355x.so (without it the prover leg is left out)")
    ap.add_argument("--out")
    ap.add_argument("--prover-leg", action="store_true", help="(internal) run the prover leg in this process")
    a = ap.parse_args()
    if a.prover_leg:
        prover_leg(a.seconds)
        return
    import torch
    from mpcith_kyber_kosk_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("tools/kem_keypair_rate.py needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    ctx = api.Kosk(kyber_k=K, max_batch=1)
    pkb, skb, ctb = ctx.pk_bytes, ctx.sk_bytes, api.ct_bytes(K)
    say("kem_keypair_rate: Kyber-768, %s, window >= %.1f s, %d repeats; items/s by stream events (by wall clock)" % (torch.cuda.get_device_name(0), a.seconds, a.repeats))
    med = {}
    for n in [int(x) for x in a.sizes.split(",")]:
        coins = hashlib.shake_256(b"keypair-rate:coins:%d" % n).digest(64 * n)
        d_coins = torch.frombuffer(bytearray(coins), dtype=torch.uint8).cuda()
        d_m = torch.frombuffer(bytearray(coins[:32 * n]), dtype=torch.uint8).cuda()
        d_pk = torch.empty(n * pkb, dtype=torch.uint8, device="cuda"); d_sk = torch.empty(n * skb, dtype=torch.uint8, device="cuda")
        d_ct = torch.empty(n * ctb, dtype=torch.uint8, device="cuda"); d_ss = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        d_flags = torch.full((n,), 0xFF, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        h = ctx.handle
        shapes = [("keypair", "device", lambda: ctx.kem_keypair(d_coins.data_ptr(), n=n, out=(d_pk.data_ptr(), d_sk.data_ptr()))),
                  ("check_sk", "device", lambda: api.lib.kosk_kem_check_sk(h, n, d_sk.data_ptr(), d_flags.data_ptr())),
                  ("kem_enc", "device", lambda: ctx.kem_enc(d_pk.data_ptr(), d_m.data_ptr(), n=n, out=(d_ct.data_ptr(), d_ss.data_ptr())))]
        if n == 4096:
            h_pk, h_sk = C.create_string_buffer(n * pkb), C.create_string_buffer(n * skb)
            shapes.append(("keypair", "host", lambda: api.lib.kosk_kem_keypair_batch(h, n, coins, h_pk, h_sk)))
        for what, where, fn in shapes:
            for _ in range(3):  # warm-up of this shape (the first call also allocates the KEM workspace)
                fn()
            if what == "check_sk":
                assert not bool(d_flags.any()), "a generated key does not pass kosk_kem_check_sk"
            runs = [window(ctx, fn, n, a.seconds) for _ in range(a.repeats)]
            med[(what, where, n)] = statistics.median(r[0] for r in runs)
            say("%-8s n %6d %-6s buffers: %s /s   median %.0f   (%d calls per window)"
                % (what, n, where, "  ".join("%.0f (%.0f)" % (r[0], r[1]) for r in runs), med[(what, where, n)], runs[0][2]))
        say("keypair / kem_enc at n %6d (medians, device buffers): %.3f" % (n, med[("keypair", "device", n)] / med[("kem_enc", "device", n)]))
        del d_coins, d_m, d_pk, d_sk, d_ct, d_ss, d_flags
    say("launch groups: kem_keypair %d kem_check %d" % (ctx.path_count(api.Kosk.PATH_KEM_KEYPAIR), ctx.path_count(api.Kosk.PATH_KEM_CHECK)))
    ctx.close()
    ref = reference_rate(a.seconds)
    if ref is None:
        say("reference baseline: oracle/_ref absent, not measured")
    else:
        say("reference (kyber/kem.c keypair_derand, one core, through ctypes): %.0f /s (%.1f us)" % (ref, 1e6 / ref))
        for (what, where, n), v in sorted(med.items()):
            if what == "keypair":
                say("ratio keypair n %6d %-6s: %.1f x one reference core" % (n, where, v / ref))
    if not a.parent_lib:
        say("(no --parent-lib: the prover leg is left out)")
    else:
        env = dict(os.environ)
        env["KOSK_LIB_PATH"] = os.path.abspath(a.parent_lib)
        rates = []
        for _ in range(a.repeats):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--prover-leg", "--seconds", str(a.seconds)], cwd=ROOT, env=env,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=300)
            if r.returncode:
                raise SystemExit("the prover leg failed (exit %d)\n%s" % (r.returncode, r.stderr[-2000:]))
            rates.append(json.loads(r.stdout.strip().splitlines()[-1])["keypairs_per_s"])
        pm = statistics.median(rates)
        say("prover path (parent library, kosk_stage_prover_inputs, %d per call, host tapes, wall clock): %s /s   median %.0f"
            % (PROVER_BATCH, "  ".join("%.0f" % x for x in rates), pm))
        for n in sorted(set(k_[2] for k_ in med)):
            say("ratio keypair n %6d device / prover path: %.1f" % (n, med[("keypair", "device", n)] / pm))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
