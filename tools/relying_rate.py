"""The relying party in numbers: paths/s of kosk_regtree_check_paths and proofs/s of
kosk_regsort_check_proofs at n = 46 / 4 096 / 65 536 and depth 10 / 16 / 20, next to one host core looping over kosk_regtree_root_from_path
and kosk_regsort_check_proof (what they replace); kosk_kem_enc_proven next to kosk_kem_enc_batch at the same n (the price of the check
inside the call); and the untouched calls kosk_kem_enc_batch, kosk_registry_prove_slots and kosk_registry_prove_absent on this tree against
the parent's library.

    python tools/relying_rate.py --parent-lib <the parent commit's libkosk_mi355x.so> [--commit <text>] [--reps 15]
                                 [--out profiles/relying_rate.txt]

The method of tools/monitor_rate.py: whole calls that end in a synchronisation, timed on the wall clock, each shape warmed up, median of
--reps; inputs and outputs in device memory, so that a call is its launches and not PCIe.  Each leg runs in a fresh child process of this
one (`--worker`), one after the other:
    old      the PARENT commit's library (KOSK_LIB_PATH): the three untouched calls.  It runs first twice, then alternates with `new`: the
             spread of its medians between runs is the yardstick
    new      this tree, the same calls
    relying  this tree: a registrar of 2^depth slots with 65 536 keys (as many as the table holds at depth 10) hands out paths and absence
             records; a second handle without a registry checks them.  The verdicts are compared with the host functions' on the first
             4 096 items of every shape before anything is timed
"""
import argparse
import ctypes as C
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K = 2
NS = (46, 4096, 65536)
DEPTHS = (10, 16, 20)
HOST_ITEMS = 4096
EXISTING_CAPACITY = 1 << 16


def wall_us(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def median_us(fn, reps):
    fn(); fn()
    return statistics.median(wall_us(fn) for _ in range(reps))


def p(t_, off=0):
    return C.c_void_p(t_.data_ptr() + off)


def registrar(api, torch, k, capacity, keys, gen):
    """a registrar handle with `keys` random keys in the first slots of a table of `capacity` -> (ctx, d_pk)"""
    lib, pkb = api.lib, api.pk_bytes(k)
    ctx = api.Kosk(kyber_k=k, max_batch=1)
    ctx.registry_reserve(capacity)
    d_pk = torch.randint(0, 256, (keys * pkb,), dtype=torch.uint8, device="cuda", generator=gen)
    slots = (C.c_int32 * keys)(*range(keys))
    torch.cuda.synchronize()
    for first in range(0, keys, 16384):
        cnt = min(16384, keys - first)
        assert lib.kosk_registry_admit(ctx.handle, cnt, p(d_pk, first * pkb), None, C.byref(slots, 4 * first)) == 0, lib.kosk_last_error(ctx.handle)
    return ctx, d_pk


def relying_worker(a):
    import torch
    from mpcith_kyber_kosk_amd import api
    k, lib = K, api.lib
    pkb, ctb = api.pk_bytes(k), api.ct_bytes(k)
    gen = torch.Generator(device="cuda").manual_seed(20410)
    out = {"box": "%s, %s" % (socket.gethostname(), torch.cuda.get_device_name(0))}
    nmax = max(NS)
    rel = api.Kosk(kyber_k=k, max_batch=1)
    rh = rel.handle
    for depth in DEPTHS:
        capacity = 1 << depth
        keys = min(nmax, capacity)
        reg, d_pk = registrar(api, torch, k, capacity, keys, gen)
        h = reg.handle
        rec = api.regsort_proof_bytes(depth)
        u8 = lambda n_: torch.zeros((max(n_, 1),), dtype=torch.uint8, device="cuda")
        d_slots = torch.arange(nmax, dtype=torch.int32, device="cuda") % keys
        slots_h = (C.c_int32 * nmax)(*[b % keys for b in range(nmax)])
        d_state, d_h, d_paths, d_root, d_ok = u8(nmax), u8(nmax * 32), u8(nmax * depth * 32), u8(32), u8(nmax)
        assert lib.kosk_registry_prove_slots(h, nmax, slots_h, (C.c_char * nmax)(), p(d_h), p(d_paths), p(d_root)) == 0, lib.kosk_last_error(h)
        # every 5th item tampered: a check does the same work whatever it finds
        d_paths.view(nmax, depth * 32)[::5, 7] ^= 1
        d_x = torch.randint(0, 256, (nmax * 32,), dtype=torch.uint8, device="cuda", generator=gen)
        d_x.view(nmax, 32)[::3] = d_h.view(nmax, 32)[::3]  # a third of the queries are enrolled
        d_kind, d_rec, d_sroot, d_verdict = u8(nmax), u8(nmax * rec), u8(32), u8(nmax)
        torch.cuda.synchronize()
        assert lib.kosk_registry_prove_absent(h, nmax, p(d_x), p(d_kind), p(d_rec), p(d_sroot)) == 0, lib.kosk_last_error(h)
        d_rec.view(nmax, rec)[::5, 20] ^= 1
        torch.cuda.synchronize()
        root, sroot = bytes(d_root.cpu().tolist()), bytes(d_sroot.cpu().tolist())
        # the host functions on the first HOST_ITEMS items: the verdicts to compare with, and one core's rate
        m = HOST_ITEMS
        hs, paths = bytes(d_h[:m * 32].cpu().tolist()), bytes(d_paths[:m * depth * 32].cpu().tolist())
        xs, recs = bytes(d_x[:m * 32].cpu().tolist()), bytes(d_rec[:m * rec].cpu().tolist())
        got = C.create_string_buffer(32)
        t0 = time.perf_counter()
        want_ok = []
        for b in range(m):
            r = lib.kosk_regtree_root_from_path(k, depth, slots_h[b], hs[32 * b:32 * b + 32], paths[32 * depth * b:32 * depth * (b + 1)], got)
            want_ok.append(1 if r == 0 and got.raw == root else 0)
        host_paths_us = (time.perf_counter() - t0) * 1e6
        t0 = time.perf_counter()
        want_v = [lib.kosk_regsort_check_proof(k, depth, xs[32 * b:32 * b + 32], recs[rec * b:rec * (b + 1)], sroot) for b in range(m)]
        host_proofs_us = (time.perf_counter() - t0) * 1e6
        out["host %d" % depth] = {"items": m, "paths_us": host_paths_us, "proofs_us": host_proofs_us}
        for n in NS:
            check = lambda: lib.kosk_regtree_check_paths(rh, n, depth, p(d_slots), None, p(d_h), p(d_paths), root, p(d_ok))
            proofs = lambda: lib.kosk_regsort_check_proofs(rh, n, depth, p(d_x), p(d_rec), sroot, p(d_verdict))
            assert check() == 0 and proofs() == 0, lib.kosk_last_error(rh)
            lim = min(n, m)
            assert d_ok[:lim].cpu().tolist() == want_ok[:lim] and d_verdict[:lim].cpu().tolist() == want_v[:lim], (depth, n)
            assert 0 in want_ok[:lim] and 1 in want_ok[:lim]
            out["paths %d %d" % (depth, n)] = median_us(check, a.reps)
            out["proofs %d %d" % (depth, n)] = median_us(proofs, a.reps)
        if depth == DEPTHS[1]:  # the fused call next to the plain one, same keys, same coins
            d_coins = torch.randint(0, 256, (nmax * 32,), dtype=torch.uint8, device="cuda", generator=gen)
            d_ct, d_ss, d_done, d_ct2, d_ss2 = u8(nmax * ctb), u8(nmax * 32), u8(nmax), u8(nmax * ctb), u8(nmax * 32)
            torch.cuda.synchronize()
            for n in NS:
                plain = lambda: lib.kosk_kem_enc_batch(rh, n, p(d_pk), p(d_coins), p(d_ct2), p(d_ss2))
                proven = lambda: lib.kosk_kem_enc_proven(rh, n, depth, p(d_pk), p(d_slots), p(d_paths), root, p(d_coins), p(d_ct), p(d_ss), p(d_done))
                assert plain() == 0 and proven() == 0, lib.kosk_last_error(rh)
                done = d_done[:n].bool()
                assert d_done[:min(n, m)].cpu().tolist() == want_ok[:min(n, m)]
                assert torch.equal(d_ct.view(nmax, ctb)[:n][done], d_ct2.view(nmax, ctb)[:n][done]) and not d_ct.view(nmax, ctb)[:n][~done].any()
                assert torch.equal(d_ss.view(nmax, 32)[:n][done], d_ss2.view(nmax, 32)[:n][done]) and not d_ss.view(nmax, 32)[:n][~done].any()
                v = []
                for _ in range(a.reps):  # alternating, so that both see the same machine
                    v.append((wall_us(plain), wall_us(proven)))
                out["enc %d" % n] = [statistics.median(x[0] for x in v), statistics.median(x[1] for x in v)]
        reg.close()
    rel.close()
    print("RESULT " + json.dumps(out), flush=True)


def existing_worker(a):
    """one library, one process: the three untouched calls at n = 4 096 on a full registry of 65 536 -> {"what": [three interleaved medians]}"""
    import torch
    from mpcith_kyber_kosk_amd import api
    k, capacity, n = K, EXISTING_CAPACITY, 4096
    lib, pkb, ctb = api.lib, api.pk_bytes(k), api.ct_bytes(k)
    gen = torch.Generator(device="cuda").manual_seed(20411)
    reg, d_pk = registrar(api, torch, k, capacity, capacity, gen)
    h = reg.handle
    depth = api.registry_tree_depth(capacity)
    rec = api.regsort_proof_bytes(depth)
    u8 = lambda n_: torch.zeros((n_,), dtype=torch.uint8, device="cuda")
    slots = (C.c_int32 * n)(*[(b * 13) % capacity for b in range(n)])
    state = (C.c_char * n)()
    d_h, d_paths, d_x, d_kind, d_rec = u8(n * 32), u8(n * depth * 32), torch.randint(0, 256, (n * 32,), dtype=torch.uint8, device="cuda", generator=gen), u8(n), u8(n * rec)
    d_coins = torch.randint(0, 256, (n * 32,), dtype=torch.uint8, device="cuda", generator=gen)
    d_ct, d_ss = u8(n * ctb), u8(n * 32)
    torch.cuda.synchronize()
    calls = (("kem_enc_batch 4096", lambda: lib.kosk_kem_enc_batch(h, n, p(d_pk), p(d_coins), p(d_ct), p(d_ss))),
             ("registry_prove_slots 4096", lambda: lib.kosk_registry_prove_slots(h, n, slots, state, p(d_h), p(d_paths), None)),
             ("registry_prove_absent 4096", lambda: lib.kosk_registry_prove_absent(h, n, p(d_x), p(d_kind), p(d_rec), None)))
    out = {}
    for what, fn in calls:
        assert fn() == 0, lib.kosk_last_error(h)
        fn()
        v = [wall_us(fn) for _ in range(3 * a.reps)]
        out[what] = [statistics.median(v[i::3]) for i in range(3)]
    reg.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(a, mode, lib_path):
    env = dict(os.environ)
    env.pop("KOSK_LIB_PATH", None)
    if lib_path:
        env["KOSK_LIB_PATH"] = os.path.abspath(lib_path)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--reps", str(a.reps)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    for ln in r.stdout.splitlines():
        if ln.startswith("RESULT "):
            return json.loads(ln[7:])
    raise SystemExit("worker %s failed (exit %d):\n%s" % (mode, r.returncode, r.stdout[-3000:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="the parent commit's libkosk_mi355x.so: the yardstick")
    ap.add_argument("--commit", default="", help="what to call this tree in the report (default: git describe of the checkout)")
    ap.add_argument("--reps", type=int, default=15, help="wall-clock repetitions of a call")
    ap.add_argument("--skip-existing", action="store_true", help="the relying party's leg alone")
    ap.add_argument("--out")
    ap.add_argument("--worker", default="", choices=["", "old", "new", "relying"], help="(internal) measure in this process and print one JSON line")
    a = ap.parse_args()
    if a.worker == "relying":
        return relying_worker(a)
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
    med = statistics.median
    res = run_worker(a, "relying", None)
    say("relying_rate: tree %s on %s" % (commit, res["box"]))
    say("-- kosk_regtree_check_paths / kosk_regsort_check_proofs, Kyber-512, every array in device memory, every 5th item tampered: wall clock"
        " of a whole call, median of %d; host: one core looping over kosk_regtree_root_from_path / kosk_regsort_check_proof through ctypes on"
        " %d of the same items (its verdicts are what the GPU's were compared with)" % (a.reps, HOST_ITEMS))
    for depth in DEPTHS:
        hr = res["host %d" % depth]
        say("depth %2d  host, one core: %8.0f paths/s  %8.0f proofs/s" % (depth, hr["items"] / hr["paths_us"] * 1e6, hr["items"] / hr["proofs_us"] * 1e6))
        for n in NS:
            pu, qu = res["paths %d %d" % (depth, n)], res["proofs %d %d" % (depth, n)]
            say("depth %2d  n %6d  paths %9.0f us = %10.0f paths/s (x %6.1f of the host core)  |  proofs %9.0f us = %10.0f proofs/s (x %6.1f)"
                % (depth, n, pu, n / pu * 1e6, (n / pu) / (hr["items"] / hr["paths_us"]), qu, n / qu * 1e6, (n / qu) / (hr["items"] / hr["proofs_us"])))
    say("-- kosk_kem_enc_proven next to kosk_kem_enc_batch, depth %d, the same keys and coins in device memory, alternating calls, median of %d"
        " (ct and ss of the proven items equal, those of the tampered ones zero: checked)" % (DEPTHS[1], a.reps))
    for n in NS:
        plain, proven = res["enc %d" % n]
        say("n %6d  kem_enc_batch %9.0f us  kem_enc_proven %9.0f us  = %.3f  (+ %.0f us for fingerprint, check and mask)" % (n, plain, proven, proven / plain, proven - plain))
    if not a.skip_existing:
        olds = [run_worker(a, "old", a.parent_lib), run_worker(a, "old", a.parent_lib)]
        news = [run_worker(a, "new", None)]
        olds.append(run_worker(a, "old", a.parent_lib))
        news.append(run_worker(a, "new", None))
        say("-- the untouched calls on a full registry of 65 536, us per call (lower is better): this tree against the parent's library,"
            " alternating processes (parent, parent, tree, parent, tree); the yardstick is the spread of the parent's medians between its own runs")
        outside = 0
        for name in olds[0]:
            y = [med(o[name]) for o in olds]
            t = [med(o[name]) for o in news]
            spread = max(y) - min(y)
            ok = med(t) <= med(y) + spread
            outside += not ok
            say("%-28s parent medians %s (spread %.1f) | tree medians %s  = %.3f  %s"
                % (name, " ".join("%.1f" % v for v in y), spread, " ".join("%.1f" % v for v in t), med(t) / med(y), "inside" if ok else "OUTSIDE the parent's spread"))
        say("result: %d of %d existing legs outside the parent's run-to-run spread" % (outside, len(olds[0])))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
