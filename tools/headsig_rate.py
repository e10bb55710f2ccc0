"""Signed heads in numbers: key generation on the GPU at heights 10, 15 and 20 next to
kosk_headsig_public_from_seed on one host core; kosk_registry_history_sign_head; kosk_headsig_verify_heads at n = 1, 46 and 4 096 next to a
host core looping over kosk_headsig_verify; and the untouched calls kosk_registry_history_head, kosk_regtree_check_paths and bench.py on
this tree against the parent's library.

    python tools/headsig_rate.py --parent-lib <the parent commit's libkosk_mi355x.so> [--commit <text>] [--reps 15]
                                 [--out profiles/headsig_rate.txt]

The method of tools/relying_rate.py: whole calls that end in a synchronisation, timed on the wall clock, each shape warmed up, median of
--reps.  Each leg runs in a fresh child process of this one (`--worker`), one after the other:
    keygen H  this tree: kosk_registry_signer_reserve at height H, under a time limit of its own (--keygen-limit seconds).  A leg that does
              not finish inside its limit ENDS THE RUN: what was measured so far and a "did not finish" line are printed and written to
              --out, the exit status is 3, and no further GPU process is started (a child killed at its limit may have left the card
              hung; this tool cannot tell slow from hung).  The limit is not raised; the remaining legs are a run of their own
    signing   this tree: sign_head on a history of 1 000 events, verify_heads with the arrays in device memory; the verdicts are compared
              with the host function's before anything is timed
    old, new  the PARENT commit's library (KOSK_LIB_PATH) and this tree: the two untouched calls.  The parent runs first twice, then
              alternates with the tree: the spread of its medians between runs is the yardstick.  bench.py alternates in the same order
"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K = 2
HEIGHTS = (10, 15, 20)
NS = (1, 46, 4096)
PERMS_PER_LEAF = 34 * 256 + 10
SEED, ID = bytes(range(32)), bytes(range(16))


def wall_us(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def median_us(fn, reps):
    fn(); fn()
    return statistics.median(wall_us(fn) for _ in range(reps))


def p(t_, off=0):
    return C.c_void_p(t_.data_ptr() + off)


def signer(api, height, events=0):
    import hashlib
    ctx = api.Kosk(kyber_k=K, max_batch=1)
    ctx.registry_reserve(max(events, 4))
    ctx.registry_history_reserve(max(events, 4))
    t0 = time.perf_counter()
    pub = ctx.registry_signer_reserve(height, SEED, ID)
    sec = time.perf_counter() - t0
    if events:
        pks = [hashlib.shake_256(b"headsig-rate:%d" % i).digest(api.pk_bytes(K)) for i in range(events)]
        ctx.registry_admit(pks, list(range(events)))
    return ctx, pub, sec


def keygen_worker(a):
    import torch
    from mpcith_kyber_kosk_amd import api
    warm, _, _ = signer(api, 5)  # the runtime's first launch is not key generation
    warm.close()
    secs = []
    for _ in range(3 if a.height <= 15 else 1):
        ctx, pub, sec = signer(api, a.height)
        launches = ctx.path_count(api.Kosk.PATH_HEADSIG_LEAVES), ctx.path_count(api.Kosk.PATH_HEADSIG_TREE)
        ctx.close()
        secs.append(sec)
    print("RESULT " + json.dumps({"sec": secs, "pub": pub.hex(), "launches": launches}), flush=True)


def signing_worker(a):
    import torch
    from mpcith_kyber_kosk_amd import api
    lib = api.lib
    out = {"device": torch.cuda.get_device_name(0)}
    t0 = time.perf_counter()
    host_pub = api.headsig_public_from_seed(10, SEED, ID)
    out["host keygen 10"] = time.perf_counter() - t0
    events = 1000
    ctx, pub, _ = signer(api, 10, events)
    assert pub == host_pub
    h = ctx.handle
    sb = api.headsig_sig_bytes(10)
    nmax = max(NS)
    sig, root = C.create_string_buffer(sb), C.create_string_buffer(32)
    sizes = [(b * 7) % (events + 1) for b in range(nmax)]
    state = {"i": 0}

    def sign():  # a different size every call: the frontier kernel runs too, as it does for a registrar
        state["i"] += 1
        return lib.kosk_registry_history_sign_head(h, sizes[state["i"] % nmax], sig, root, None)
    assert sign() == 0, lib.kosk_last_error(h)
    out["sign"] = median_us(sign, 4 * a.reps)
    out["sign same size"] = median_us(lambda: lib.kosk_registry_history_sign_head(h, 777, sig, root, None), 4 * a.reps)
    distinct = {}
    for s in sorted(set(sizes[:64])):
        g, r, _ = ctx.registry_history_sign_head(s)
        distinct[s] = (g, r)
    sizes = [sizes[b % 64] for b in range(nmax)]
    sigs = [bytearray(distinct[s][0]) for s in sizes]
    for b in range(0, nmax, 5):
        sigs[b][100 + b % 1000] ^= 1  # every 5th item tampered
    roots = b"".join(distinct[s][1] for s in sizes)
    blob = b"".join(bytes(g) for g in sigs)
    t0 = time.perf_counter()
    want = [lib.kosk_headsig_verify(pub, K, roots[32 * b:32 * b + 32], sizes[b], blob[sb * b:sb * (b + 1)]) for b in range(nmax)]
    out["host verify"] = {"items": nmax, "us": (time.perf_counter() - t0) * 1e6}
    assert set(want) == {0, 1}
    d_roots = torch.frombuffer(bytearray(roots), dtype=torch.uint8).cuda()
    d_sigs = torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    d_sizes = torch.tensor(sizes, dtype=torch.int32, device="cuda")
    d_ok = torch.zeros((nmax,), dtype=torch.uint8, device="cuda")
    gate = api.Kosk(kyber_k=K, max_batch=1)
    torch.cuda.synchronize()
    for n in NS:
        verify = lambda: lib.kosk_headsig_verify_heads(gate.handle, n, pub, p(d_roots), p(d_sizes), p(d_sigs), p(d_ok))
        assert verify() == 0, lib.kosk_last_error(gate.handle)
        assert d_ok[:n].cpu().tolist() == want[:n], n
        out["verify %d" % n] = median_us(verify, a.reps)
    gate.close()
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def existing_worker(a):
    """one library, one process: the two untouched calls -> {"what": [three interleaved medians]}"""
    import hashlib
    import torch
    from mpcith_kyber_kosk_amd import api
    lib = api.lib
    events, n, depth = 1000, 4096, 16
    ctx = api.Kosk(kyber_k=K, max_batch=1)
    ctx.registry_reserve(events)
    ctx.registry_history_reserve(events)
    pks = [hashlib.shake_256(b"headsig-rate:%d" % i).digest(api.pk_bytes(K)) for i in range(events)]
    ctx.registry_admit(pks, list(range(events)))
    h = ctx.handle
    root = C.create_string_buffer(32)
    state = {"i": 0}

    def head():
        state["i"] += 1
        return lib.kosk_registry_history_head(h, 1 + (state["i"] * 7) % events, root, None)
    gen = torch.Generator(device="cuda").manual_seed(20420)
    d_slots = torch.arange(n, dtype=torch.int32, device="cuda")
    d_h = torch.randint(0, 256, (n * 32,), dtype=torch.uint8, device="cuda", generator=gen)
    d_paths = torch.randint(0, 256, (n * depth * 32,), dtype=torch.uint8, device="cuda", generator=gen)
    d_ok = torch.zeros((n,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    calls = (("registry_history_head", head),
             ("regtree_check_paths 4096", lambda: lib.kosk_regtree_check_paths(h, n, depth, p(d_slots), None, p(d_h), p(d_paths), bytes(32), p(d_ok))))
    out = {}
    for what, fn in calls:
        assert fn() == 0, lib.kosk_last_error(h)
        fn()
        v = [wall_us(fn) for _ in range(3 * a.reps)]
        out[what] = [statistics.median(v[i::3]) for i in range(3)]
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def child_env(lib_path):
    env = dict(os.environ)
    env.pop("KOSK_LIB_PATH", None)
    if lib_path:
        env["KOSK_LIB_PATH"] = os.path.abspath(lib_path)
    return env


class LegTimeout(Exception):
    """a child was killed at its time limit: nothing more may be started on the GPU in this run"""


def run_worker(a, mode, lib_path, extra=(), limit=900):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--reps", str(a.reps)] + list(extra)
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=child_env(lib_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
    except subprocess.TimeoutExpired:
        raise LegTimeout("%s %s did not finish inside %d s: not measured (the limit was not raised); the run ends here" % (mode, " ".join(extra), limit))
    for ln in r.stdout.splitlines():
        if ln.startswith("RESULT "):
            return json.loads(ln[7:])
    raise SystemExit("worker %s failed (exit %d):\n%s" % (mode, r.returncode, r.stdout[-3000:]))


def run_bench(a, lib_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(a.bench_steps), "--warmup", str(a.bench_warmup)]
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=child_env(lib_path), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    except subprocess.TimeoutExpired:
        raise LegTimeout("bench.py did not finish inside 900 s: not measured; the run ends here")
    for ln in reversed(r.stdout.splitlines()):
        if ln.startswith("{"):
            return json.loads(ln)
    raise SystemExit("bench.py failed (exit %d):\n%s" % (r.returncode, r.stdout[-3000:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="the parent commit's libkosk_mi355x.so: the yardstick")
    ap.add_argument("--commit", default="", help="what to call this tree in the report (default: git describe of the checkout)")
    ap.add_argument("--reps", type=int, default=15, help="wall-clock repetitions of a call")
    ap.add_argument("--keygen-limit", type=int, default=120, help="seconds a key generation leg may take")
    ap.add_argument("--skip-existing", action="store_true", help="the new calls' legs alone")
    ap.add_argument("--skip-bench", action="store_true")
    ap.add_argument("--bench-steps", type=int, default=3600)
    ap.add_argument("--bench-warmup", type=int, default=180)
    ap.add_argument("--out")
    ap.add_argument("--height", type=int, default=10, help="(internal) the keygen worker's height")
    ap.add_argument("--worker", default="", choices=["", "old", "new", "keygen", "signing"], help="(internal) measure in this process and print one JSON line")
    a = ap.parse_args()
    if a.worker == "keygen":
        return keygen_worker(a)
    if a.worker == "signing":
        return signing_worker(a)
    if a.worker:
        return existing_worker(a)
    if not a.skip_existing and (not a.parent_lib or not os.path.exists(a.parent_lib)):
        raise SystemExit("--parent-lib: the parent commit's library is the yardstick of this tool")
    commit = a.commit
    if not commit:
        r = subprocess.run(["git", "describe", "--always", "--dirty"], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
        commit = r.stdout.strip() or "unknown"
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    try:
        measure(a, commit, say)
        status = 0
    except LegTimeout as e:
        say(str(e))
        status = 3
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return status


def measure(a, commit, say):
    med = statistics.median
    sg = run_worker(a, "signing", None)
    host10 = sg["host keygen 10"]
    first = True
    stopped = None
    say("headsig_rate: tree %s on one MI355X (the runtime names it %s)" % (commit, sg["device"]))
    for height in HEIGHTS:
        try:
            res = run_worker(a, "keygen", None, ["--height", str(height)], limit=a.keygen_limit)
        except LegTimeout as e:  # the legs measured before it are still reported below; nothing more is started
            stopped = e
            break
        perms = (1 << height) * PERMS_PER_LEAF + (1 << height) - 1
        host = host10 * (1 << (height - 10))
        if first:
            say("-- kosk_registry_signer_reserve: wall clock of the whole call (allocation, every leaf launch, the tree's tiers, the root to the"
                " host), a fresh handle each time, best of %d after a warm-up handle; host: kosk_headsig_public_from_seed on one core at height"
                " 10 (%.2f s, the same public key), SCALED by 2^(h - 10) for the other heights" % (len(res["sec"]), host10))
            first = False
        sec = min(res["sec"])
        say("height %2d  %10.4f s  %8.2f G permutations/s  (%d leaf launches, %d tree launches)  |  host, one core%s: %9.1f s  (x %.0f)"
            % (height, sec, perms / sec / 1e9, res["launches"][0], res["launches"][1], "" if height == 10 else ", scaled", host, host / sec))
    say("-- kosk_registry_history_sign_head at height 10 on a history of 1 000 events, signature and root to host memory, median of %d:"
        " %.0f us a head of a new size (the frontier kernel included), %.0f us at a size signed before" % (4 * a.reps, sg["sign"], sg["sign same size"]))
    hv = sg["host verify"]
    host_rate = hv["items"] / hv["us"] * 1e6
    say("-- kosk_headsig_verify_heads at height 10, arrays in device memory, every 5th item tampered, verdicts equal to the host function's on"
        " every item; host: one core looping over kosk_headsig_verify through ctypes on %d items: %.0f heads/s" % (hv["items"], host_rate))
    for n in NS:
        us = sg["verify %d" % n]
        say("n %5d  %9.0f us = %9.0f heads/s  (x %.1f of the host core)" % (n, us, n / us * 1e6, n / us * 1e6 / host_rate))
    if stopped:
        raise stopped
    if not a.skip_existing:
        olds = [run_worker(a, "old", a.parent_lib), run_worker(a, "old", a.parent_lib)]
        news = [run_worker(a, "new", None)]
        olds.append(run_worker(a, "old", a.parent_lib))
        news.append(run_worker(a, "new", None))
        say("-- the untouched calls, us per call (lower is better): this tree against the parent's library, alternating processes (parent,"
            " parent, tree, parent, tree); the yardstick is the spread of the parent's medians between its own runs")
        outside = 0
        for name in olds[0]:
            y = [med(o[name]) for o in olds]
            t = [med(o[name]) for o in news]
            spread = max(y) - min(y)
            ok = med(t) <= med(y) + spread
            outside += not ok
            say("%-28s parent medians %s (spread %.1f) | tree medians %s  = %.3f  %s"
                % (name, " ".join("%.1f" % v for v in y), spread, " ".join("%.1f" % v for v in t), med(t) / med(y), "inside" if ok else "OUTSIDE the parent's spread"))
        if not a.skip_bench:
            order = [a.parent_lib, a.parent_lib, None, a.parent_lib, None]
            runs = [(lp, run_bench(a, lp)) for lp in order]
            key = "value" if "value" in runs[0][1] else sorted(k for k, v in runs[0][1].items() if isinstance(v, (int, float)))[0]
            y = [r[key] for lp, r in runs if lp]
            t = [r[key] for lp, r in runs if not lp]
            spread = max(y) - min(y)
            ok = med(t) >= med(y) - spread
            outside += not ok
            say("bench.py --steps %d --warmup %d, %s (higher is better): parent %s (spread %.0f) | tree %s  = %.3f  %s"
                % (a.bench_steps, a.bench_warmup, key, " ".join("%.0f" % v for v in y), spread, " ".join("%.0f" % v for v in t), med(t) / med(y),
                   "inside" if ok else "OUTSIDE the parent's spread"))
        say("result: %d existing legs outside the parent's run-to-run spread" % outside)


if __name__ == "__main__":
    sys.exit(main())
