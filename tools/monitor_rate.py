"""The registry monitor in numbers: events/s of kosk_monitor_feed at capacities 2^16 and 2^20 with a
checkpoint every 1, 64 and 16 384 events; the same replay on one host core with the library's host functions, roots compared; and the
existing calls that the monitor's refactor sits under -- kosk_registry_root, kosk_registry_sorted_root, kosk_registry_history_checkpoint and
a one-key kosk_registry_admit with a history -- on this tree against the parent's library.

    python tools/monitor_rate.py --parent-lib <the parent commit's libkosk_mi355x.so> [--commit <text>] [--events 65536] [--reps 15]
                                 [--out profiles/monitor_rate.txt]

The method of tools/registry_sorted_rate.py: whole calls that end in a synchronisation, timed on the wall clock, each shape warmed up,
median of --reps.  Each leg runs in a fresh child process of this one (`--worker`), one after the other:
    old      the PARENT commit's library (KOSK_LIB_PATH): the four existing calls.  It runs first twice, then alternates with `new`: the
             spread of its medians between runs is the yardstick
    new      this tree, the same calls
    monitor  this tree: the log is made by a registrar handle (the same keys admitted over the same slots again and again, so every key is
             an EVICT and an ADMIT, and a checkpoint at the stated distance), read once with kosk_registry_history_read and fed from host
             memory in calls of 16 384 events
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
CAPACITIES = (1 << 16, 1 << 20)
EVERY = (1, 64, 16384)
EXISTING_CAPACITY = 1 << 16
E = 80


def wall_us(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e6


def make_log(api, torch, k, capacity, events, every, gen):
    """a registrar's log of about `events` events on a table of `capacity`: one admission of `batch` keys over the first slots per round
    (an ADMIT each in the first round, an EVICT and an ADMIT each later) and a checkpoint every `every` events -> the raw records"""
    lib, pkb = api.lib, api.pk_bytes(k)
    p = lambda t_: C.c_void_p(t_.data_ptr())
    ctx = api.Kosk(kyber_k=k, max_batch=1)
    h = ctx.handle
    ctx.registry_reserve(capacity)
    ctx.registry_history_reserve(events + 2 * every + 8)
    batch = max(1, min(every, capacity, 16384) // 2)
    d_keys = torch.randint(0, 256, (batch * pkb,), dtype=torch.uint8, device="cuda", generator=gen)
    slots = (C.c_int32 * batch)(*range(batch))
    torch.cuda.synchronize()
    while ctx.registry_history_level()[0] < events:
        assert lib.kosk_registry_admit(h, batch, p(d_keys), None, slots) == 0, lib.kosk_last_error(h)
        ctx.registry_history_checkpoint()
        if every == 1:  # one key into the empty slot 0 and out again: every call appends one event
            ctx.registry_evict([0])
            ctx.registry_history_checkpoint()
    n = ctx.registry_history_level()[0]
    buf = C.create_string_buffer(E * n)
    assert lib.kosk_registry_history_read(h, 0, n, buf) == 0
    head = ctx.registry_history_head()[0]
    roots = (ctx.registry_root()[0], ctx.registry_sorted_root()[0])
    ctx.close()
    return buf.raw, n, head, roots


def host_replay(api, k, capacity, log, n):
    """the sequential replay on one host core: the table in numpy, the two roots recomputed at every checkpoint with
    kosk_host_sha3_256_multi (the auditor of examples/registry_history.cpp, every checkpoint instead of one) -> checkpoints verified"""
    import numpy as np
    from tools.registry_sorted_rate import host_sorted_root
    lib = api.lib
    d = api.registry_tree_depth(capacity)
    state = np.zeros(capacity, np.uint8)
    hs = np.zeros((capacity, 32), np.uint8)
    rec = np.frombuffer(log, np.uint8).reshape(n, E)
    ops = rec[:, 0:4].copy().view("<u4").ravel()
    slots = rec[:, 4:8].copy().view("<u4").ravel()
    tag = np.frombuffer(b"kosk-regtree-v1", np.uint8)
    empty = np.frombuffer(api.regtree_leaf(k), np.uint8)
    seen = 0
    for i in range(n):
        op, s = int(ops[i]), int(slots[i])
        if op == 1:
            assert not state[s]
            state[s] = 1; hs[s] = rec[i, 16:48]
        elif op == 2:
            assert state[s] and (hs[s] == rec[i, 16:48]).all()
            state[s] = 0; hs[s] = 0
        else:
            level = np.tile(empty, (1 << d, 1))
            occ = np.nonzero(state)[0]
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
            assert level[0].tobytes() == rec[i, 16:48].tobytes(), "the host's slot root and the log's disagree"
            assert host_sorted_root(api, k, capacity, state, hs) == rec[i, 48:80].tobytes(), "the host's sorted root and the log's disagree"
            assert int(slots[i]) == int(state.sum())
            seen += 1
    return seen


def monitor_worker(a):
    import torch
    from mpcith_kyber_kosk_amd import api
    k = K
    lib = api.lib
    gen = torch.Generator(device="cuda").manual_seed(20401)
    out = {"box": "%s, %s" % (socket.gethostname(), torch.cuda.get_device_name(0))}
    for capacity in CAPACITIES:
        for every in EVERY:
            events = a.events if every > 1 else max(64, a.events // 256)  # a full sort per event: fewer events
            log, n, head, roots = make_log(api, torch, k, capacity, events, every, gen)
            ctx = api.Kosk(kyber_k=k, max_batch=1)
            h = ctx.handle
            bad, why = C.c_int(), C.c_int()

            def feed():
                assert lib.kosk_monitor_reserve(h, capacity, n) == 0, lib.kosk_last_error(h)
                t0 = time.perf_counter()
                for first in range(0, n, 16384):
                    cnt = min(16384, n - first)
                    assert lib.kosk_monitor_feed(h, cnt, log[first * E:(first + cnt) * E], C.byref(bad), C.byref(why)) == 1, (bad.value, why.value)
                return (time.perf_counter() - t0) * 1e6
            feed()
            assert ctx.monitor_head() == (head, n) and ctx.monitor_roots() == roots
            us = [feed() for _ in range(min(a.reps, 5))]
            ids = [ctx.path_count(i) for i in (42, 43, 44, 45)]
            ctx.close()
            host_n = min(n, 2 * (every + 1))  # two checkpoints: one core hashes 2^(D + 2) nodes at each
            t0 = time.perf_counter()
            cps = host_replay(api, k, capacity, log[:host_n * E], host_n)
            host_us = (time.perf_counter() - t0) * 1e6
            out["feed %d %d" % (capacity, every)] = {"events": n, "us": statistics.median(us), "launches": ids, "host_events": host_n, "host_checkpoints": cps,
                                                      "host_us": host_us}
    print("RESULT " + json.dumps(out), flush=True)


def existing_worker(a):
    """one library, one process: the four existing calls on a full registry of 65 536 with a history -> {"what": [three interleaved medians]}"""
    import torch
    from mpcith_kyber_kosk_amd import api
    k, capacity = K, EXISTING_CAPACITY
    lib, pkb = api.lib, api.pk_bytes(k)
    p = lambda t_: C.c_void_p(t_.data_ptr())
    gen = torch.Generator(device="cuda").manual_seed(20402)
    ctx = api.Kosk(kyber_k=k, max_batch=1)
    h = ctx.handle
    ctx.registry_reserve(capacity)
    ctx.registry_history_reserve(capacity + 16 * a.reps + 64)
    d_keys = torch.randint(0, 256, (capacity * pkb,), dtype=torch.uint8, device="cuda", generator=gen)
    every = (C.c_int32 * capacity)(*range(capacity))
    one = (C.c_int32 * 1)(5)
    torch.cuda.synchronize()
    for first in range(0, capacity, 16384):
        assert lib.kosk_registry_admit(h, 16384, C.c_void_p(d_keys.data_ptr() + first * pkb), None, C.byref(every, 4 * first)) == 0, lib.kosk_last_error(h)
    root = C.create_string_buffer(32)
    idx = C.c_int()
    admit = lambda: lib.kosk_registry_admit(h, 1, p(d_keys), None, one)  # replaces the key of slot 5: an EVICT and an ADMIT, both trees stale
    calls = (("admit 1 key with a history", admit, None), ("root", lambda: lib.kosk_registry_root(h, root, None, None), admit),
             ("sorted_root", lambda: lib.kosk_registry_sorted_root(h, root, None, None), admit),
             ("history_checkpoint", lambda: lib.kosk_registry_history_checkpoint(h, C.byref(idx)), admit))
    out = {}
    for what, fn, before in calls:
        v = []
        for i in range(a.reps + 2):
            if before:
                assert before() == 0, lib.kosk_last_error(h)
            us = wall_us(lambda: fn())
            if i >= 2:
                v.append(us)
        out[what] = [statistics.median(v[i::3]) for i in range(3)]
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(a, mode, lib_path):
    env = dict(os.environ)
    env.pop("KOSK_LIB_PATH", None)
    if lib_path:
        env["KOSK_LIB_PATH"] = os.path.abspath(lib_path)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--events", str(a.events), "--reps", str(a.reps)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    for ln in r.stdout.splitlines():
        if ln.startswith("RESULT "):
            return json.loads(ln[7:])
    raise SystemExit("worker %s failed (exit %d):\n%s" % (mode, r.returncode, r.stdout[-3000:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="the parent commit's libkosk_mi355x.so: the yardstick")
    ap.add_argument("--commit", default="", help="what to call this tree in the report (default: git describe of the checkout)")
    ap.add_argument("--events", type=int, default=65536, help="events of a fed log (a checkpoint after every event: 1 / 256 of it)")
    ap.add_argument("--reps", type=int, default=15, help="wall-clock repetitions of a call")
    ap.add_argument("--skip-existing", action="store_true", help="the monitor's leg alone")
    ap.add_argument("--out")
    ap.add_argument("--worker", default="", choices=["", "old", "new", "monitor"], help="(internal) measure in this process and print one JSON line")
    a = ap.parse_args()
    if a.worker == "monitor":
        return monitor_worker(a)
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
    res = run_worker(a, "monitor", None)
    say("monitor_rate: tree %s on %s" % (commit, res["box"]))
    say("-- kosk_monitor_feed, Kyber-512, a registrar's log fed from host memory in calls of 16 384 events: wall clock from the first feed to"
        " the last one's return, median; head and both roots are the registrar's (checked); host: the same replay on one core, table in"
        " numpy, both roots recomputed at every checkpoint with kosk_host_sha3_256_multi and compared (a prefix of the log where stated)")
    for capacity in CAPACITIES:
        for every in EVERY:
            r = res["feed %d %d" % (capacity, every)]
            say("capacity %7d  a checkpoint every %5d  %6d events  %10.0f us = %9.0f events/s  (launches: %d keys, %d apply, %d leaves, %d check)"
                " | host, one core: %d events with %d checkpoints %10.0f us = %8.0f events/s"
                % (capacity, every, r["events"], r["us"], r["events"] / r["us"] * 1e6, *r["launches"], r["host_events"], r["host_checkpoints"], r["host_us"],
                   r["host_events"] / r["host_us"] * 1e6))
    if not a.skip_existing:
        olds = [run_worker(a, "old", a.parent_lib), run_worker(a, "old", a.parent_lib)]
        news = [run_worker(a, "new", None)]
        olds.append(run_worker(a, "old", a.parent_lib))
        news.append(run_worker(a, "new", None))
        say("-- the refactored existing calls on a full registry of 65 536 with a history, us per call (lower is better): this tree against the"
            " parent's library, alternating processes (parent, parent, tree, parent, tree); the yardstick is the spread of the parent's medians"
            " between its own runs")
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
