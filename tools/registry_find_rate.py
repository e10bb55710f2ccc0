"""The registry by fingerprint in numbers: kosk_kem_enc_peers next to kosk_kem_enc_slots on the same items,
kosk_registry_find alone, a rebuild of the index, enrolments next to admissions, and the existing calls kosk_kem_enc_slots and
kosk_registry_admit on this tree against the parent's library.  Kyber-768, a registry of 65 536 distinct keys.

    python tools/registry_find_rate.py --parent-lib <the parent commit's libkosk_mi355x.so> [--sizes 46,4096,65536] [--seconds 0.5]
                                       [--repeats 3] [--out profiles/registry_find_rate.txt]

The method of tools/registry_rate.py: every buffer of the timed calls resident in HBM (torch tensors handed over as device pointers), each
shape warmed up, then whole calls counted inside a window of at least --seconds between two events on the handle's stream, --repeats
times, median.  Rebuilds and enrolments are host-visible calls with host outputs and are timed on the wall clock.  Each leg runs in a fresh
child process of this one (`--worker`), one after the other:
    old    the PARENT commit's library (KOSK_LIB_PATH): kosk_kem_enc_slots over n distinct slots and kosk_registry_admit of n keys.  It
           runs first twice, then alternates with `new`: the spread of its medians between runs is the yardstick
    new    this tree, the same two calls
    peers  this tree: kosk_kem_enc_peers and kosk_kem_enc_slots on the same items in the same process, kosk_registry_find, the rebuild at a
           full and at a half-evicted registry, kosk_registry_enrol next to kosk_registry_admit
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
K = 3
CAPACITY = 65536


def window(ctx, call, n, seconds):
    calls = 0
    ctx.timer_start()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        call()
        calls += 1
    return n * calls / (ctx.timer_stop_ms() * 1e-3)


def wall_us(fn, reps):
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e6)
    return statistics.median(t)


def worker(a):
    """one library, one process: {"what n": [rates]} as one JSON line"""
    import torch
    from mpcith_kyber_kosk_amd import api
    ctx = api.Kosk(kyber_k=K, max_batch=1)
    lib, h, ctb, pkb = api.lib, ctx.handle, api.ct_bytes(K), api.pk_bytes(K)
    dev = lambda blob: torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    p = lambda t_: C.c_void_p(t_.data_ptr())
    sizes = [int(x) for x in a.sizes.split(",")]
    # 65 536 distinct records: kosk_registry_admit makes no encoding check, any bytes are a key
    blob = hashlib.shake_256(b"registry-find-rate:keys").digest(CAPACITY * pkb)
    d_all = dev(blob)
    torch.cuda.synchronize()
    every = (C.c_int32 * CAPACITY)(*[(7 * b + 3) % CAPACITY for b in range(CAPACITY)])  # key b lives in slot (7 b + 3) mod 65 536
    ctx.registry_reserve(CAPACITY)
    assert lib.kosk_registry_admit(h, CAPACITY, p(d_all), None, every) == 0, lib.kosk_last_error(h)
    out = {}
    for n in sizes:
        coins = b"".join(hashlib.shake_256(b"registry-find-rate:m:%d" % b).digest(32) for b in range(n))
        d_m = dev(coins)
        d_ct = torch.empty(n * ctb, dtype=torch.uint8, device="cuda"); d_ss = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        d_done = torch.empty(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        digest = lambda: hashlib.sha3_256(bytes(d_ct.cpu().numpy()) + bytes(d_ss.cpu().numpy())).hexdigest()
        keys = [(11 * b + 5) % CAPACITY for b in range(n)]  # item b goes to key keys[b]: neighbours in the batch are not neighbours in HBM
        slots = (C.c_int32 * n)(*[every[i] for i in keys])
        shapes = [("enc_slots", lambda: lib.kosk_kem_enc_slots(h, n, slots, p(d_m), p(d_ct), p(d_ss), p(d_done)))]
        if a.worker == "peers":
            d_h = dev(b"".join(hashlib.sha3_256(blob[i * pkb:(i + 1) * pkb]).digest() for i in keys))
            d_found = torch.empty(n, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            shapes += [("enc_peers", lambda: lib.kosk_kem_enc_peers(h, n, p(d_h), p(d_m), p(d_ct), p(d_ss), p(d_done))),
                       ("find", lambda: lib.kosk_registry_find(h, n, p(d_h), p(d_found)))]
        else:
            d_pk = dev(b"".join(blob[i * pkb:(i + 1) * pkb] for i in keys))
            torch.cuda.synchronize()
            shapes += [("admit", lambda: lib.kosk_registry_admit(h, n, p(d_pk), None, slots))]  # every call replaces the same n keys by themselves
        for what, fn in shapes:
            for _ in range(3):
                assert fn() == 0, (what, n, lib.kosk_last_error(h))
            if what in ("enc_slots", "enc_peers"):
                out["digest %s %d" % (what, n)] = digest()
            if what == "find":
                assert d_found.cpu().tolist() == list(slots), "kosk_registry_find disagrees with the slots the keys went to"
            out["%s %d" % (what, n)] = [window(ctx, fn, n, a.seconds) for _ in range(a.repeats)]
    if a.worker == "peers":
        # a rebuild: replace one key by itself (the index is invalid), then look one fingerprint up; minus the two calls on their own
        one_pk, one_slot = dev(blob[:pkb]), (C.c_int32 * 1)(every[0])
        one_h, one_found = dev(hashlib.sha3_256(blob[:pkb]).digest()), torch.empty(1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        admit1 = lambda: lib.kosk_registry_admit(h, 1, p(one_pk), None, one_slot)
        find1 = lambda: lib.kosk_registry_find(h, 1, p(one_h), p(one_found))

        def both():
            assert admit1() == 0 and find1() == 0
        for label in ("full", "half"):
            if label == "half":
                ctx.registry_evict([every[b] for b in range(1, CAPACITY, 2)])
                assert ctx.registry_level() == (CAPACITY // 2, CAPACITY)
            both()
            t_both, t_admit, t_find = wall_us(both, 30), wall_us(admit1, 30), wall_us(find1, 30)
            out["rebuild %s" % label] = [t_both, t_admit, t_find]
        out["paths"] = [ctx.path_count(i) for i in (api.Kosk.PATH_REGISTRY_INDEX, api.Kosk.PATH_REGISTRY_FIND, api.Kosk.PATH_KEM_ENC_PEERS, 28)]
        # enrolments next to admissions: n new keys into the empty registry, evicted again outside the clock
        ctx.registry_evict(list(every))
        for n in sizes:
            d_pk = dev(blob[:n * pkb])
            torch.cuda.synchronize()
            got, status = (C.c_int32 * n)(), C.create_string_buffer(n)
            first = (C.c_int32 * n)(*range(n))
            t_enrol, t_admit = [], []
            for _ in range(5):
                t0 = time.perf_counter()
                assert lib.kosk_registry_enrol(h, n, p(d_pk), None, got, status) == 0, lib.kosk_last_error(h)
                t_enrol.append(time.perf_counter() - t0)
                assert list(got) == list(first) and status.raw == b"\x01" * n
                ctx.registry_evict(list(first))
                t0 = time.perf_counter()
                assert lib.kosk_registry_admit(h, n, p(d_pk), None, first) == 0
                t_admit.append(time.perf_counter() - t0)
                ctx.registry_evict(list(first))
            out["enrol %d" % n] = [n / statistics.median(t_enrol[1:]), n / statistics.median(t_admit[1:])]
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(a, mode, lib_path):
    env = dict(os.environ)
    env.pop("KOSK_LIB_PATH", None)
    if lib_path:
        env["KOSK_LIB_PATH"] = os.path.abspath(lib_path)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--sizes", a.sizes, "--seconds", str(a.seconds), "--repeats", str(a.repeats)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    for ln in r.stdout.splitlines():
        if ln.startswith("RESULT "):
            return json.loads(ln[7:])
    raise SystemExit("worker %s failed (exit %d):\n%s" % (mode, r.returncode, r.stdout[-3000:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="the parent commit's libkosk_mi355x.so: the yardstick")
    ap.add_argument("--sizes", default="46,4096,65536")
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--worker", default="", choices=["", "old", "new", "peers"], help="(internal) measure in this process and print one JSON line")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's library is the yardstick of this tool")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    med = statistics.median
    sizes = [int(x) for x in a.sizes.split(",")]
    say("registry_find_rate: Kyber-768, a registry of %d distinct keys; window >= %.1f s, %d repeats; items/s by stream events, device buffers"
        % (CAPACITY, a.seconds, a.repeats))
    olds = [run_worker(a, "old", a.parent_lib), run_worker(a, "old", a.parent_lib)]
    news = [run_worker(a, "new", None)]
    olds.append(run_worker(a, "old", a.parent_lib))
    news.append(run_worker(a, "new", None))
    peers = run_worker(a, "peers", None)
    say("-- kosk_kem_enc_peers next to kosk_kem_enc_slots on the same items, one process (the same ct and ss: checked)")
    for n in sizes:
        assert peers["digest enc_peers %d" % n] == peers["digest enc_slots %d" % n] == olds[0]["digest enc_slots %d" % n], "the legs disagree on ct / ss"
        s, q, f = peers["enc_slots %d" % n], peers["enc_peers %d" % n], peers["find %d" % n]
        say("n %6d  enc_slots %s median %.0f = %.1f us per call | enc_peers %s median %.0f = %.1f us per call | peers / slots %.3f, + %.1f us per call"
            % (n, " ".join("%.0f" % v for v in s), med(s), n / med(s) * 1e6, " ".join("%.0f" % v for v in q), med(q), n / med(q) * 1e6, med(q) / med(s),
               (n / med(q) - n / med(s)) * 1e6))
        say("n %6d  kosk_registry_find (copy in, k_registry_find, copy out, one synchronisation) %s median %.0f lookups/s = %.1f us per call"
            % (n, " ".join("%.0f" % v for v in f), med(f), n / med(f) * 1e6))
    say("-- a rebuild (hipMemsetAsync of %d entries + k_registry_index + synchronisation), wall clock, median of 30: admit of one key + find of one"
        " fingerprint, minus the two calls on their own" % (4 * CAPACITY // 2))
    for label in ("full", "half"):
        b, t_a, t_f = peers["rebuild %s" % label]
        say("registry %s: admit + find %.1f us, admit alone (+ the rebuild's cause) %.1f us, find alone %.1f us: rebuild = %.1f us" % (label, b, t_a, t_f, b - t_a - t_f))
    say("launches of k_registry_index %d, of k_registry_find %d, launch groups kem_enc_peers %d, kem_enc_slots %d in that process" % tuple(peers["paths"]))
    say("-- enrolments (kosk_registry_enrol: hash, find, 36 bytes per key to the host, resolve, admit) next to kosk_registry_admit, n new keys"
        " into an empty registry, wall clock, median of 4")
    for n in sizes:
        e, ad = peers["enrol %d" % n]
        say("n %6d  enrol %.0f keys/s | admit %.0f keys/s | enrol / admit %.2f" % (n, e, ad, e / ad))
    say("-- the existing calls: this tree against the parent's library, alternating processes (parent, parent, tree, parent, tree); the"
        " yardstick is the spread of the parent's medians between its own runs")
    outside = 0
    for n in sizes:
        for what in ("enc_slots", "admit"):
            y = [med(o["%s %d" % (what, n)]) for o in olds]
            t = [med(o["%s %d" % (what, n)]) for o in news]
            spread = max(y) - min(y)
            ok = med(t) >= med(y) - spread
            outside += not ok
            say("%-9s n %6d  parent medians %s (spread %.0f) | tree medians %s  = %.3f  %s"
                % (what, n, " ".join("%.0f" % v for v in y), spread, " ".join("%.0f" % v for v in t), med(t) / med(y),
                   "inside" if ok else "BELOW the parent's spread"))
    say("result: %d of %d existing legs below the parent's run-to-run spread" % (outside, 2 * len(sizes)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
