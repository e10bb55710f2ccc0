"""The sorted tree (format kosk-regsort-v1) in numbers: full rebuilds at capacities 2^10, 2^16 and 2^20, nearly empty
and full, under each setting of the sort (records a tile, steps a launch above the tile, threads of the tile kernel);
the slot tree's full rebuild at the same sizes in the same process; the same sorted trees on one host core (a sort and the hashing: the auditor's recomputation, whose root the tool compares with the GPU's);
proofs per second of kosk_registry_prove_absent next to kosk_registry_prove_peers; and the existing calls kosk_registry_root,
kosk_registry_prove_slots, kosk_registry_find and kosk_registry_admit on this tree against the parent's library.

    python tools/registry_sorted_rate.py --parent-lib <the parent commit's libkosk_mi355x.so> [--commit <text>] [--sizes 46,4096,65536]
                                         [--seconds 0.3] [--repeats 3] [--out profiles/registry_sorted_rate.txt]

The method of tools/registry_tree_rate.py: the buffers of the timed calls resident in HBM, each shape warmed up, whole calls counted inside a
window of at least --seconds between two events on the handle's stream, --repeats times, median.  A rebuild is a host-visible call that ends
in a synchronisation and is timed on the wall clock around kosk_registry_sorted_root / kosk_registry_root, median of --reps.  Each leg runs in
a fresh child process of this one (`--worker`), one after the other:
    old     the PARENT commit's library (KOSK_LIB_PATH): the slot tree's rebuilds, prove_slots, find and admit.  It runs first twice, then
            alternates with `new`: the spread of its medians between runs is the yardstick
    new     this tree, the same calls
    sorted  this tree: the sorted rebuilds, the proofs and the host alternative, Kyber-512 (the smallest slot: 2^20 of them take 3 GB)
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
CAPACITIES = (1 << 10, 1 << 16, 1 << 20)
PROOF_CAPACITY = 1 << 16
# KOSK_DEBUG_REGSORT_TILE_LG (records a tile, as a logarithm), KOSK_DEBUG_REGSORT_STEP2 (two steps above the tile in a launch),
# KOSK_DEBUG_REGSORT_TILE_THREADS (the tile kernel's block)
SETTINGS = ((11, 1, 1024), (11, 0, 1024), (10, 1, 1024), (12, 1, 1024), (11, 1, 512), (11, 1, 256), (10, 1, 256), (12, 1, 256))  # the build's first
ENV = ("KOSK_DEBUG_REGSORT_TILE_LG", "KOSK_DEBUG_REGSORT_STEP2", "KOSK_DEBUG_REGSORT_TILE_THREADS")
TAG = b"kosk-regsort-v1"


def window(ctx, call, n, seconds):
    calls = 0
    ctx.timer_start()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        call()
        calls += 1
    return n * calls / (ctx.timer_stop_ms() * 1e-3)


def wall_us(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def host_sorted_root(api, k, capacity, state, hs):
    """kosk-regsort-v1 on one host core: a sort of the occupied slots by (fingerprint, slot), then the hashing with
    kosk_host_sha3_256_multi; state uint8[capacity], hs uint8[capacity, 32] -> the root"""
    import numpy as np
    lib = api.lib
    d = api.registry_tree_depth(capacity)
    occ = np.nonzero(state)[0]
    level = np.tile(np.frombuffer(api.regsort_leaf(k), np.uint8), (1 << d, 1))
    tag = np.frombuffer(TAG, np.uint8)
    if len(occ):
        words = hs[occ].view(">u8")  # memcmp order = the order of four big-endian words
        order = occ[np.lexsort((occ, words[:, 3], words[:, 2], words[:, 1], words[:, 0]))]
        msg = np.zeros((len(order), 56), np.uint8)
        msg[:, :15] = tag; msg[:, 16:48] = hs[order]; msg[:, 48:52] = order.astype("<u4").view(np.uint8).reshape(-1, 4); msg[:, 52] = k
        out = np.empty((len(order), 32), np.uint8)
        lib.kosk_host_sha3_256_multi(out.ctypes.data, msg.ctypes.data, 56, 56, len(order), 1)
        level[:len(order)] = out
    for _ in range(d):
        m = len(level) // 2
        msg = np.empty((m, 80), np.uint8)
        msg[:, :15] = tag; msg[:, 15] = 2; msg[:, 16:] = level.reshape(m, 64)
        level = np.empty((m, 32), np.uint8)
        lib.kosk_host_sha3_256_multi(level.ctypes.data, msg.ctypes.data, 80, 80, m, 1)
    return level[0].tobytes()


def registry_of(api, torch, k, capacity, full, gen):
    """a handle with a registry of `capacity`, every slot occupied or one key per 1 024 slots; `touch` replaces those keys by themselves, so
    that the next call rebuilds both trees whole"""
    lib, pkb = api.lib, api.pk_bytes(k)
    p = lambda t_: C.c_void_p(t_.data_ptr())
    subtrees = max(1, capacity >> 10)
    ctx = api.Kosk(kyber_k=k, max_batch=1)
    h = ctx.handle
    ctx.registry_reserve(capacity)
    d_touch = torch.randint(0, 256, (subtrees * pkb,), dtype=torch.uint8, device="cuda", generator=gen)
    touch_slots = (C.c_int32 * subtrees)(*[q * 1024 for q in range(subtrees)])
    if full:
        d_keys = torch.randint(0, 256, (capacity * pkb,), dtype=torch.uint8, device="cuda", generator=gen)
        every = (C.c_int32 * capacity)(*range(capacity))
        torch.cuda.synchronize()
        assert lib.kosk_registry_admit(h, capacity, p(d_keys), None, every) == 0, lib.kosk_last_error(h)
        del d_keys
    torch.cuda.synchronize()
    touch = lambda: lib.kosk_registry_admit(h, subtrees, p(d_touch), None, touch_slots)
    assert touch() == 0, lib.kosk_last_error(h)
    return ctx, touch, (d_touch,)


def sorted_worker(a):
    import numpy as np
    import torch
    from mpcith_kyber_kosk_amd import api
    k = K
    lib = api.lib
    p = lambda t_: C.c_void_p(t_.data_ptr())
    med = statistics.median
    gen = torch.Generator(device="cuda").manual_seed(20261)
    out = {"box": "%s, %s" % (socket.gethostname(), torch.cuda.get_device_name(0))}
    root = C.create_string_buffer(32)
    for capacity in CAPACITIES:
        every = (C.c_int32 * capacity)(*range(capacity))
        for label in ("sparse", "full"):
            ctx, touch, keep = registry_of(api, torch, k, capacity, label == "full", gen)
            h = ctx.handle

            def sorted_root():
                assert lib.kosk_registry_sorted_root(h, root, None, None) == 0, lib.kosk_last_error(h)
                return root.raw

            def slot_root():
                assert lib.kosk_registry_root(h, root, None, None) == 0, lib.kosk_last_error(h)
            for name in ENV:
                os.environ.pop(name, None)
            want = sorted_root()
            slot_root()
            ids = [ctx.path_count(i) for i in (api.Kosk.PATH_REGSORT_SORT, api.Kosk.PATH_REGSORT_TREE)]
            rebuild = {s: [] for s in SETTINGS}
            slot_tree, current = [], []
            for _ in range(a.reps):  # the settings and the two trees alternate inside one process
                for s in SETTINGS:
                    os.environ.update(zip(ENV, map(str, s)))
                    assert touch() == 0
                    rebuild[s].append(wall_us(sorted_root))
                    assert root.raw == want, "a setting of the sort changes the root"
                    current.append(wall_us(sorted_root))
                    slot_tree.append(wall_us(slot_root))
            for name in ENV:
                os.environ.pop(name, None)
            used = ctx.registry_level()[0]
            # what the auditor holds: every slot's state and fingerprint (kosk_registry_prove_slots delivers them a launch group at a time)
            state = np.zeros(capacity, np.uint8)
            hs = np.zeros((capacity, 32), np.uint8)
            group = min(capacity, 16384)
            d_paths = torch.empty(group * api.registry_tree_depth(capacity) * 32, dtype=torch.uint8, device="cuda")
            for first in range(0, capacity, group):
                assert lib.kosk_registry_prove_slots(h, group, C.byref(every, 4 * first), state[first:].ctypes.data, hs[first:].ctypes.data,
                                                     p(d_paths), None) == 0, lib.kosk_last_error(h)
            del d_paths
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                got = host_sorted_root(api, k, capacity, state, hs)
                host.append((time.perf_counter() - t0) * 1e6)
            assert got == want, "the host's sorted tree and the GPU's disagree"
            out["rebuild %d %s" % (capacity, label)] = {"used": used, "sorted": {"%d/%d/%d" % s: med(v) for s, v in rebuild.items()}, "slot": med(slot_tree),
                                                          "current": med(current), "host": med(host), "launches": ids}
            if capacity == PROOF_CAPACITY and label == "full":
                d = api.registry_tree_depth(capacity)
                rec = api.regsort_proof_bytes(d)
                for n in [int(x) for x in a.sizes.split(",")]:
                    keys = [(11 * b + 5) % capacity for b in range(n)]
                    q = hs[keys].copy()
                    q[1::2, 31] ^= 1  # every second query is a neighbour of an enrolled key: absent
                    d_q = torch.from_numpy(q).cuda()
                    d_kind = torch.empty(n, dtype=torch.uint8, device="cuda"); d_rec = torch.empty(n * rec, dtype=torch.uint8, device="cuda")
                    d_root = torch.empty(32, dtype=torch.uint8, device="cuda"); d_slots = torch.empty(n, dtype=torch.int32, device="cuda")
                    d_done = torch.empty(n, dtype=torch.uint8, device="cuda"); d_paths = torch.empty(n * d * 32, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    shapes = [("prove_absent", lambda: lib.kosk_registry_prove_absent(h, n, p(d_q), p(d_kind), p(d_rec), p(d_root))),
                              ("prove_peers", lambda: lib.kosk_registry_prove_peers(h, n, p(d_q), p(d_slots), p(d_paths), p(d_done), p(d_root)))]
                    for what, fn in shapes:
                        for _ in range(3):
                            assert fn() == 0, (what, n, lib.kosk_last_error(h))
                        if what == "prove_absent":
                            kinds, recs = bytes(d_kind.cpu().numpy()), bytes(d_rec.cpu().numpy())
                            assert kinds == bytes(2 - b % 2 for b in range(n)) and bytes(d_root.cpu().numpy()) == want
                            for b in (0, 1, n // 2, n - 1):  # the host verifier on a sample
                                assert api.regsort_check_proof(k, d, q[b].tobytes(), recs[rec * b:rec * (b + 1)], want) == kinds[b]
                        out["%s %d" % (what, n)] = [window(ctx, fn, n, a.seconds) for _ in range(a.repeats)]
            ctx.close()
            del keep
    print("RESULT " + json.dumps(out), flush=True)


def neighbours_worker(a):
    """one library, one process: the slot tree's full rebuild at each capacity, then prove_slots, find and admit at each n on a full registry
    of 65 536 -> {"what n": [values]}"""
    import torch
    from mpcith_kyber_kosk_amd import api
    k = K
    lib, pkb = api.lib, api.pk_bytes(k)
    p = lambda t_: C.c_void_p(t_.data_ptr())
    gen = torch.Generator(device="cuda").manual_seed(20262)
    root = C.create_string_buffer(32)
    out = {}
    for capacity in CAPACITIES:
        ctx, touch, keep = registry_of(api, torch, k, capacity, True, gen)
        h = ctx.handle
        assert lib.kosk_registry_root(h, root, None, None) == 0
        v = []
        for _ in range(a.reps):
            assert touch() == 0
            v.append(wall_us(lambda: lib.kosk_registry_root(h, root, None, None)))
        out["root %d" % capacity] = [statistics.median(v[i::3]) for i in range(3)]  # three interleaved medians
        if capacity == PROOF_CAPACITY:
            d = api.registry_tree_depth(capacity)
            for n in [int(x) for x in a.sizes.split(",")]:
                keys = [(11 * b + 5) % capacity for b in range(n)]
                slots = (C.c_int32 * n)(*keys)
                d_h = torch.empty(n * 32, dtype=torch.uint8, device="cuda"); d_paths = torch.empty(n * d * 32, dtype=torch.uint8, device="cuda")
                d_found = torch.empty(n, dtype=torch.int32, device="cuda")
                d_pk = torch.randint(0, 256, (n * pkb,), dtype=torch.uint8, device="cuda", generator=gen)
                state = C.create_string_buffer(n)
                torch.cuda.synchronize()
                assert lib.kosk_registry_admit(h, n, p(d_pk), None, slots) == 0
                shapes = [("prove_slots", lambda: lib.kosk_registry_prove_slots(h, n, slots, state, p(d_h), p(d_paths), None)),
                          ("find", lambda: lib.kosk_registry_find(h, n, p(d_h), p(d_found))),  # d_h: what prove_slots left there
                          ("admit", lambda: lib.kosk_registry_admit(h, n, p(d_pk), None, slots))]  # every call replaces the same n keys by themselves
                for what, fn in shapes:
                    for _ in range(3):
                        assert fn() == 0, (what, n, lib.kosk_last_error(h))
                    if what == "find":
                        assert d_found.cpu().tolist() == keys
                    out["%s %d" % (what, n)] = [window(ctx, fn, n, a.seconds) for _ in range(a.repeats)]
        ctx.close()
        del keep
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(a, mode, lib_path):
    env = dict(os.environ)
    env.pop("KOSK_LIB_PATH", None)
    for name in ENV:
        env.pop(name, None)
    if lib_path:
        env["KOSK_LIB_PATH"] = os.path.abspath(lib_path)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--sizes", a.sizes, "--seconds", str(a.seconds), "--repeats", str(a.repeats),
           "--reps", str(a.reps)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    for ln in r.stdout.splitlines():
        if ln.startswith("RESULT "):
            return json.loads(ln[7:])
    raise SystemExit("worker %s failed (exit %d):\n%s" % (mode, r.returncode, r.stdout[-3000:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="the parent commit's libkosk_mi355x.so: the yardstick")
    ap.add_argument("--commit", default="", help="what to call this tree in the report (default: git describe of the checkout)")
    ap.add_argument("--sizes", default="46,4096,65536")
    ap.add_argument("--seconds", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15, help="wall-clock repetitions of a rebuild")
    ap.add_argument("--out")
    ap.add_argument("--worker", default="", choices=["", "old", "new", "sorted"], help="(internal) measure in this process and print one JSON line")
    a = ap.parse_args()
    if a.worker == "sorted":
        return sorted_worker(a)
    if a.worker:
        return neighbours_worker(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
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
    sizes = [int(x) for x in a.sizes.split(",")]
    res = run_worker(a, "sorted", None)
    say("registry_sorted_rate: tree %s on %s" % (commit, res["box"]))
    say("-- rebuilds, Kyber-512: wall clock around kosk_registry_sorted_root (keys, sort, tiers, synchronisation, 32 bytes to the host) and"
        " around kosk_registry_root after the same mutation, median of %d, us; the settings alternate in one process and give the same root"
        " (checked); the host's root is the GPU's (checked)" % a.reps)
    for capacity in CAPACITIES:
        for label in ("sparse", "full"):
            r = res["rebuild %d %s" % (capacity, label)]
            say("capacity %7d %-6s (%7d keys)  sorted rebuild by (lg of the tile / steps a launch / threads of the tile kernel) %s; the build's"
                " setting takes %d sort + %d tier launches | on a current tree %.1f | slot tree, full rebuild %.1f | host: one core, sort +"
                " hashing %.0f us"
                % (capacity, label, r["used"], "  ".join("%s: %.1f" % (s, v) for s, v in r["sorted"].items()), r["launches"][0], r["launches"][1],
                   r["current"], r["slot"], r["host"]))
    say("-- proofs, a full registry of 65 536 (D = 16: %d bytes a record, 512 a path), every second query absent, device buffers; items/s by"
        " stream events, window >= %.1f s, %d repeats" % (16 + 64 + 64 * 16, a.seconds, a.repeats))
    for n in sizes:
        for what in ("prove_absent", "prove_peers"):
            v = res["%s %d" % (what, n)]
            say("n %6d  kosk_registry_%s %s median %.0f /s = %.1f us per call" % (n, what, " ".join("%.0f" % x for x in v), med(v), n / med(v) * 1e6))
    olds = [run_worker(a, "old", a.parent_lib), run_worker(a, "old", a.parent_lib)]
    news = [run_worker(a, "new", None)]
    olds.append(run_worker(a, "old", a.parent_lib))
    news.append(run_worker(a, "new", None))
    say("-- the existing calls, Kyber-512: this tree against the parent's library, alternating processes (parent, parent, tree, parent, tree);"
        " the yardstick is the spread of the parent's medians between its own runs.  root: us per full rebuild (lower is better);"
        " the others: items/s on a full registry of 65 536 (higher is better)")
    outside, legs = 0, 0
    names = [("root %d" % c, True) for c in CAPACITIES] + [("%s %d" % (w, n), False) for n in sizes for w in ("prove_slots", "find", "admit")]
    for name, lower in names:
        y = [med(o[name]) for o in olds]
        t = [med(o[name]) for o in news]
        spread = max(y) - min(y)
        ok = med(t) <= med(y) + spread if lower else med(t) >= med(y) - spread
        outside += not ok
        legs += 1
        say("%-18s parent medians %s (spread %.1f) | tree medians %s  = %.3f  %s"
            % (name, " ".join("%.1f" % v for v in y), spread, " ".join("%.1f" % v for v in t), med(t) / med(y),
               "inside" if ok else "OUTSIDE the parent's spread"))
    say("result: %d of %d existing legs outside the parent's run-to-run spread" % (outside, legs))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
