"""The registry tree (format kosk-regtree-v1) in numbers: full rebuilds at capacities 2^10, 2^16 and 2^20, sparse and
full, under each setting of the wave-sponge tail; the rebuild after one admission; paths per second; the same trees built on one host core
after fetching the fingerprints (what a caller had before); and the existing calls kosk_registry_find, kosk_kem_enc_peers and
kosk_registry_admit on this tree against the parent's library.

    python tools/registry_tree_rate.py --parent-lib <the parent commit's libkosk_mi355x.so> [--commit <text>] [--sizes 46,4096,65536]
                                       [--seconds 0.3] [--repeats 3] [--out profiles/registry_tree_rate.txt]

The method of tools/registry_find_rate.py: the buffers of the timed calls resident in HBM, each shape warmed up, whole calls counted inside a
window of at least --seconds between two events on the handle's stream, --repeats times, median.  A rebuild is a host-visible call that ends
in a synchronisation and is timed on the wall clock around kosk_registry_root, median of --reps.  Each leg runs in a fresh child process of
this one (`--worker`), one after the other:
    old    the PARENT commit's library (KOSK_LIB_PATH): kosk_registry_find, kosk_kem_enc_peers and kosk_registry_admit, Kyber-768, 65 536 keys.
           It runs first twice, then alternates with `new`: the spread of its medians between runs is the yardstick
    new    this tree, the same three calls
    tree   this tree: the rebuilds, the paths and the host alternative, Kyber-512 (the smallest slot: 2^20 of them take 3 GB)
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K = 3
CAPACITY = 65536
TREE_K = 2
TREE_CAPACITIES = (1 << 10, 1 << 16, 1 << 20)
TAILS = (0, 8, 32, 64)  # KOSK_DEBUG_REGTREE_WAVE_TAIL: levels of this many nodes or fewer on the wave sponge
TAG = b"kosk-regtree-v1"


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


def neighbours_worker(a):
    """one library, one process: find, enc_peers and admit at each n -> {"what n": [rates]}"""
    import torch
    from mpcith_kyber_kosk_amd import api
    ctx = api.Kosk(kyber_k=K, max_batch=1)
    lib, h, ctb, pkb = api.lib, ctx.handle, api.ct_bytes(K), api.pk_bytes(K)
    dev = lambda blob: torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    p = lambda t_: C.c_void_p(t_.data_ptr())
    sizes = [int(x) for x in a.sizes.split(",")]
    blob = hashlib.shake_256(b"registry-tree-rate:keys").digest(CAPACITY * pkb)
    d_all = dev(blob)
    torch.cuda.synchronize()
    every = (C.c_int32 * CAPACITY)(*[(7 * b + 3) % CAPACITY for b in range(CAPACITY)])
    ctx.registry_reserve(CAPACITY)
    assert lib.kosk_registry_admit(h, CAPACITY, p(d_all), None, every) == 0, lib.kosk_last_error(h)
    out = {}
    for n in sizes:
        d_m = dev(b"".join(hashlib.shake_256(b"registry-tree-rate:m:%d" % b).digest(32) for b in range(n)))
        d_ct = torch.empty(n * ctb, dtype=torch.uint8, device="cuda"); d_ss = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        d_done = torch.empty(n, dtype=torch.uint8, device="cuda"); d_found = torch.empty(n, dtype=torch.int32, device="cuda")
        keys = [(11 * b + 5) % CAPACITY for b in range(n)]
        slots = (C.c_int32 * n)(*[every[i] for i in keys])
        d_h = dev(b"".join(hashlib.sha3_256(blob[i * pkb:(i + 1) * pkb]).digest() for i in keys))
        d_pk = dev(b"".join(blob[i * pkb:(i + 1) * pkb] for i in keys))
        torch.cuda.synchronize()
        shapes = [("find", lambda: lib.kosk_registry_find(h, n, p(d_h), p(d_found))),
                  ("enc_peers", lambda: lib.kosk_kem_enc_peers(h, n, p(d_h), p(d_m), p(d_ct), p(d_ss), p(d_done))),
                  ("admit", lambda: lib.kosk_registry_admit(h, n, p(d_pk), None, slots))]  # every call replaces the same n keys by themselves
        for what, fn in shapes:
            for _ in range(3):
                assert fn() == 0, (what, n, lib.kosk_last_error(h))
            if what == "find":
                assert d_found.cpu().tolist() == list(slots)
            if what == "enc_peers":
                out["digest %d" % n] = hashlib.sha3_256(bytes(d_ct.cpu().numpy()) + bytes(d_ss.cpu().numpy())).hexdigest()
            out["%s %d" % (what, n)] = [window(ctx, fn, n, a.seconds) for _ in range(a.repeats)]
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def host_tree(api, k, capacity, state, hs):
    """kosk-regtree-v1 on one host core with kosk_host_sha3_256_multi: state uint8[capacity], hs uint8[capacity, 32] -> the root"""
    import numpy as np
    lib = api.lib
    d = api.registry_tree_depth(capacity)
    level = np.tile(np.frombuffer(api.regtree_leaf(k), np.uint8), (1 << d, 1))
    occ = np.nonzero(state)[0]
    tag = np.frombuffer(TAG, np.uint8)
    if len(occ):
        msg = np.zeros((len(occ), 52), np.uint8)
        msg[:, :15] = tag; msg[:, 16:48] = hs[occ]; msg[:, 48] = k
        out = np.empty((len(occ), 32), np.uint8)
        lib.kosk_host_sha3_256_multi(out.ctypes.data, msg.ctypes.data, 52, 52, len(occ), 1)
        level[occ] = out
    for _ in range(d):
        m = len(level) // 2
        msg = np.empty((m, 80), np.uint8)
        msg[:, :15] = tag; msg[:, 15] = 2; msg[:, 16:] = level.reshape(m, 64)
        level = np.empty((m, 32), np.uint8)
        lib.kosk_host_sha3_256_multi(level.ctypes.data, msg.ctypes.data, 80, 80, m, 1)
    return level[0].tobytes()


def tree_worker(a):
    import numpy as np
    import torch
    from mpcith_kyber_kosk_amd import api
    k = TREE_K
    lib, pkb = api.lib, api.pk_bytes(k)
    p = lambda t_: C.c_void_p(t_.data_ptr())
    med = statistics.median
    gen = torch.Generator(device="cuda").manual_seed(20251)
    out = {"box": "%s, %s" % (socket.gethostname(), torch.cuda.get_device_name(0))}
    root = C.create_string_buffer(32)
    ctx, h = None, None

    def get_root():
        assert lib.kosk_registry_root(h, root, None, None) == 0, lib.kosk_last_error(h)
        return root.raw
    for capacity in TREE_CAPACITIES:
        subtrees = max(1, capacity >> 10)
        d_keys = torch.randint(0, 256, (capacity * pkb,), dtype=torch.uint8, device="cuda", generator=gen)
        d_touch = torch.randint(0, 256, (subtrees * pkb,), dtype=torch.uint8, device="cuda", generator=gen)
        d_one = torch.randint(0, 256, (pkb,), dtype=torch.uint8, device="cuda", generator=gen)
        torch.cuda.synchronize()
        touch_slots = (C.c_int32 * subtrees)(*[q * 1024 for q in range(subtrees)])
        one_slot = (C.c_int32 * 1)(min(5, capacity - 1))
        every = (C.c_int32 * capacity)(*range(capacity))
        for label in ("sparse", "full"):
            ctx = api.Kosk(kyber_k=k, max_batch=1)  # a handle per registry: closing it frees a million slots without evicting them
            h = ctx.handle
            ctx.registry_reserve(capacity)
            if label == "full":
                assert lib.kosk_registry_admit(h, capacity, p(d_keys), None, every) == 0, lib.kosk_last_error(h)
            # one key per leaf subtree replaced by itself: every subtree is dirty, the next root is a full rebuild
            touch = lambda: lib.kosk_registry_admit(h, subtrees, p(d_touch), None, touch_slots)
            one = lambda: lib.kosk_registry_admit(h, 1, p(d_one), None, one_slot)
            assert touch() == 0 and one() == 0
            os.environ.pop("KOSK_DEBUG_REGTREE_WAVE_TAIL", None)
            want = get_root()
            full = {t: [] for t in TAILS}
            for _ in range(a.reps):  # the settings alternate inside one process
                for t in TAILS:
                    os.environ["KOSK_DEBUG_REGTREE_WAVE_TAIL"] = str(t)
                    assert touch() == 0
                    full[t].append(wall_us(get_root))
                    assert root.raw == want, "the wave-sponge tail changes the root"
            os.environ.pop("KOSK_DEBUG_REGTREE_WAVE_TAIL", None)
            after_one, current = [], []
            for _ in range(a.reps):
                assert one() == 0
                after_one.append(wall_us(get_root))
                current.append(wall_us(get_root))
            assert root.raw == want
            used = ctx.registry_level()[0]
            # the alternative: fetch every slot's state and fingerprint (kosk_registry_read), then the tree on one core
            state = np.zeros(capacity, np.uint8)
            hs = np.zeros((capacity, 32), np.uint8)
            fetch = -1.0
            if label == "full":
                fetch = wall_us(lambda: lib.kosk_registry_read(h, capacity, every, state.ctypes.data, None, hs.ctypes.data))
                out["fetch %d" % capacity] = fetch
            else:
                assert lib.kosk_registry_read(h, subtrees, touch_slots, state.ctypes.data, None, hs.ctypes.data) == 0
                st2, hs2 = np.zeros(capacity, np.uint8), np.zeros((capacity, 32), np.uint8)
                idx = np.array(list(touch_slots))
                st2[idx] = state[:subtrees]; hs2[idx] = hs[:subtrees]
                assert lib.kosk_registry_read(h, 1, one_slot, state.ctypes.data, None, hs.ctypes.data) == 0
                st2[one_slot[0]] = state[0]; hs2[one_slot[0]] = hs[0]
                state, hs = st2, hs2
            host = []
            for _ in range(3):
                t0 = time.perf_counter()
                got = host_tree(api, k, capacity, state, hs)
                host.append((time.perf_counter() - t0) * 1e6)
            assert got == want, "the host tree and the GPU tree disagree"
            out["rebuild %d %s" % (capacity, label)] = {"used": used, "full": {str(t): med(v) for t, v in full.items()}, "one": med(after_one),
                                                          "current": med(current), "host": med(host)}
            ctx.close()
    # paths: a full registry of 65 536
    capacity = 1 << 16
    d = api.registry_tree_depth(capacity)
    ctx = api.Kosk(kyber_k=k, max_batch=1)
    h = ctx.handle
    d_keys = torch.randint(0, 256, (capacity * pkb,), dtype=torch.uint8, device="cuda", generator=gen)
    ctx.registry_reserve(capacity)
    every = (C.c_int32 * capacity)(*range(capacity))
    assert lib.kosk_registry_admit(h, capacity, p(d_keys), None, every) == 0
    hs = np.zeros((capacity, 32), np.uint8)
    state = np.zeros(capacity, np.uint8)
    assert lib.kosk_registry_read(h, capacity, every, state.ctypes.data, None, hs.ctypes.data) == 0
    want = get_root()
    for n in [int(x) for x in a.sizes.split(",")]:
        keys = [(11 * b + 5) % capacity for b in range(n)]
        slots = (C.c_int32 * n)(*keys)
        d_h = torch.from_numpy(hs[keys].copy()).cuda()
        d_slots = torch.empty(n, dtype=torch.int32, device="cuda"); d_done = torch.empty(n, dtype=torch.uint8, device="cuda")
        d_paths = torch.empty(n * d * 32, dtype=torch.uint8, device="cuda"); d_root = torch.empty(32, dtype=torch.uint8, device="cuda")
        d_hout = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        state_n = C.create_string_buffer(n)
        torch.cuda.synchronize()
        shapes = [("prove_peers", lambda: lib.kosk_registry_prove_peers(h, n, p(d_h), p(d_slots), p(d_paths), p(d_done), p(d_root))),
                  ("prove_slots", lambda: lib.kosk_registry_prove_slots(h, n, slots, state_n, p(d_hout), p(d_paths), p(d_root)))]
        for what, fn in shapes:
            for _ in range(3):
                assert fn() == 0, (what, n, lib.kosk_last_error(h))
            paths = bytes(d_paths.cpu().numpy())
            for b in (0, n // 2, n - 1):  # the host verifier on a sample
                assert api.regtree_root_from_path(k, d, keys[b], hs[keys[b]].tobytes(), paths[32 * d * b:32 * d * (b + 1)]) == want
            assert bytes(d_root.cpu().numpy()) == want and (what == "prove_slots" or d_slots.cpu().tolist() == keys)
            out["%s %d" % (what, n)] = [window(ctx, fn, n, a.seconds) for _ in range(a.repeats)]
    out["paths"] = [ctx.path_count(i) for i in (api.Kosk.PATH_REGISTRY_TREE, api.Kosk.PATH_REGISTRY_SUBTREES, api.Kosk.PATH_REGISTRY_PATH)]
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(a, mode, lib_path):
    env = dict(os.environ)
    env.pop("KOSK_LIB_PATH", None)
    env.pop("KOSK_DEBUG_REGTREE_WAVE_TAIL", None)
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
    ap.add_argument("--worker", default="", choices=["", "old", "new", "tree"], help="(internal) measure in this process and print one JSON line")
    a = ap.parse_args()
    if a.worker == "tree":
        return tree_worker(a)
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
    tree = run_worker(a, "tree", None)
    say("registry_tree_rate: tree %s on %s" % (commit, tree["box"]))
    say("-- rebuilds, Kyber-512: wall clock around kosk_registry_root (tiers + synchronisation + 32 bytes to the host), median of %d, us; the"
        " settings of the wave-sponge tail alternate in one process and give the same root (checked)" % a.reps)
    for capacity in TREE_CAPACITIES:
        for label in ("sparse", "full"):
            r = tree["rebuild %d %s" % (capacity, label)]
            say("capacity %7d %-6s (%7d keys)  full rebuild, tail %s | after one admission %.1f | on a current tree %.1f | host: one core %.0f us%s"
                % (capacity, label, r["used"], "  ".join("%s: %.1f" % (t, r["full"][str(t)]) for t in TAILS), r["one"], r["current"], r["host"],
                   (" + fetching state and h slot by slot (kosk_registry_read) %.0f us" % tree["fetch %d" % capacity]) if label == "full" else ""))
    say("-- paths, a full registry of 65 536 (D = 16, 512 bytes a path), device buffers; items/s by stream events, window >= %.1f s, %d repeats"
        % (a.seconds, a.repeats))
    for n in sizes:
        for what in ("prove_peers", "prove_slots"):
            v = tree["%s %d" % (what, n)]
            say("n %6d  kosk_registry_%s %s median %.0f paths/s = %.1f us per call" % (n, what, " ".join("%.0f" % x for x in v), med(v), n / med(v) * 1e6))
    say("launches of k_registry_tree %d, leaf subtrees hashed %d, launches of k_registry_path %d in that process" % tuple(tree["paths"]))
    olds = [run_worker(a, "old", a.parent_lib), run_worker(a, "old", a.parent_lib)]
    news = [run_worker(a, "new", None)]
    olds.append(run_worker(a, "old", a.parent_lib))
    news.append(run_worker(a, "new", None))
    say("-- the existing calls, Kyber-768, 65 536 keys: this tree against the parent's library, alternating processes (parent, parent, tree,"
        " parent, tree); the yardstick is the spread of the parent's medians between its own runs")
    outside = 0
    for n in sizes:
        assert news[0]["digest %d" % n] == olds[0]["digest %d" % n], "the legs disagree on ct / ss"
        for what in ("find", "enc_peers", "admit"):
            y = [med(o["%s %d" % (what, n)]) for o in olds]
            t = [med(o["%s %d" % (what, n)]) for o in news]
            spread = max(y) - min(y)
            ok = med(t) >= med(y) - spread
            outside += not ok
            say("%-9s n %6d  parent medians %s (spread %.0f) | tree medians %s  = %.3f  %s"
                % (what, n, " ".join("%.0f" % v for v in y), spread, " ".join("%.0f" % v for v in t), med(t) / med(y),
                   "inside" if ok else "BELOW the parent's spread"))
    say("result: %d of %d existing legs below the parent's run-to-run spread" % (outside, 3 * len(sizes)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
