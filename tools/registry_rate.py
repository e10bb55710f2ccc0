"""Items/s of kosk_kem_enc_slots (the verified-key registry) next to kosk_kem_enc_batch on the same keys and
kosk_kem_enc_key, admissions per second, and the existing calls that run the touched kernels on this tree against the parent's library.
Kyber-768.

    python tools/registry_rate.py --parent-lib <the parent commit's libkosk_mi355x.so> [--sizes 46,4096,65536] [--seconds 1.0]
                                  [--repeats 3] [--out profiles/registry_rate.txt]

The method of tools/kem_onekey_rate.py: every buffer resident in HBM (torch tensors handed over as device pointers), each shape warmed
up, then whole calls counted inside a window of at least --seconds between two events on the handle's stream, --repeats times, median.
Each leg runs in a fresh child process of this one (`--worker`), one after the other:
    old   the PARENT commit's library (KOSK_LIB_PATH): kosk_kem_enc_batch on n distinct keys, kosk_kem_dec_batch, kosk_kem_enc_key,
          kosk_kem_dec_key -- the yardstick; its margin is max - min of its own repeats
    new   this tree, the same four calls
    slots this tree: kosk_kem_enc_slots over n distinct slots and with every item on one slot, kosk_registry_admit of n keys,
          kosk_registry_admit_verified of 46 keys, kosk_kem_key_set
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
KEYS = 130  # distinct key pairs; n keys are these over and over (a key's position in the batch is what the kernels see, not its value)
VERIFIED = 46


def window(ctx, call, n, seconds):
    calls = 0
    ctx.timer_start()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        call()
        calls += 1
    return n * calls / (ctx.timer_stop_ms() * 1e-3)


def worker(a):
    """one library, one process: {"what n": [rates]} as one JSON line"""
    import torch
    from mpcith_kyber_kosk_amd import api
    pairs = [api.host_keygen(K, hashlib.shake_256(b"registry-rate:kg:%d" % i).digest(64))[:2] for i in range(KEYS)]
    ctx = api.Kosk(kyber_k=K, max_batch=1)
    lib, h, ctb = api.lib, ctx.handle, api.ct_bytes(K)
    dev = lambda blob: torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    p = lambda t_: C.c_void_p(t_.data_ptr())
    out = {}
    sizes = [int(x) for x in a.sizes.split(",")]
    if a.worker == "slots":
        ctx.registry_reserve(max(sizes))
        t = []
        for _ in range(21):
            t0 = time.perf_counter()
            ctx.kem_key_set(pk=pairs[0][0])
            t.append((time.perf_counter() - t0) * 1e6)
        out["key_set_us"] = [t[0], statistics.median(t[1:]), min(t[1:]), max(t[1:])]
    else:
        ctx.kem_key_set(sk=pairs[0][1])
    for n in sizes:
        coins = b"".join(hashlib.shake_256(b"registry-rate:m:%d" % b).digest(32) for b in range(n))
        pks = b"".join(pairs[b % KEYS][0] for b in range(n))
        d_m, d_pk = dev(coins), dev(pks)
        d_ct = torch.empty(n * ctb, dtype=torch.uint8, device="cuda"); d_ss = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        d_ss2 = torch.empty(n * 32, dtype=torch.uint8, device="cuda"); d_done = torch.empty(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        digest = lambda: hashlib.sha3_256(bytes(d_ct.cpu().numpy()) + bytes(d_ss.cpu().numpy())).hexdigest()
        if a.worker == "slots":
            distinct = (C.c_int32 * n)(*[(7 * b + 3) % n if n % 7 else b for b in range(n)])  # a permutation: neighbours in the batch are not neighbours in HBM
            one = (C.c_int32 * n)(*([int(distinct[0])] * n))
            admit = lambda: lib.kosk_registry_admit(h, n, p(d_pk), None, distinct)
            shapes = [("admit", admit),
                      ("enc_slots distinct", lambda: lib.kosk_kem_enc_slots(h, n, distinct, p(d_m), p(d_ct), p(d_ss), p(d_done))),
                      ("enc_slots one", lambda: lib.kosk_kem_enc_slots(h, n, one, p(d_m), p(d_ct), p(d_ss), p(d_done)))]
        else:
            d_sk = dev(b"".join(pairs[b % KEYS][1] for b in range(n)))
            torch.cuda.synchronize()
            shapes = [("enc_batch", lambda: lib.kosk_kem_enc_batch(h, n, p(d_pk), p(d_m), p(d_ct), p(d_ss))),
                      ("dec_batch", lambda: lib.kosk_kem_dec_batch(h, n, p(d_ct), p(d_sk), p(d_ss2))),
                      ("enc_key", lambda: lib.kosk_kem_enc_key(h, n, p(d_m), p(d_ct), p(d_ss))),
                      ("dec_key", lambda: lib.kosk_kem_dec_key(h, n, p(d_ct), p(d_ss2)))]
        for what, fn in shapes:
            for _ in range(3):
                assert fn() == 0, (what, n, lib.kosk_last_error(h))
            if what in ("enc_batch", "enc_slots distinct"):
                out["digest %d" % n] = digest()  # the slot call and the per-item call on the same keys and coins: the same bytes
            if what in ("dec_batch", "dec_key"):
                assert torch.equal(d_ss, d_ss2), "dec(enc) != ss"
            out["%s %d" % (what, n)] = [window(ctx, fn, n, a.seconds) for _ in range(a.repeats)]
        if a.worker == "slots":
            assert ctx.registry_level() == (n, max(sizes))
            ctx.registry_evict(list(distinct))
    if a.worker == "slots":
        out["groups"] = [ctx.path_count(api.Kosk.PATH_REGISTRY_ADMIT), ctx.path_count(api.Kosk.PATH_KEM_ENC_SLOTS), ctx.path_count(12), ctx.path_count(20)]
        ctx.close()
        # the keys of a verify call: max_batch = 46, the line of record
        ctx = api.Kosk(kyber_k=K, max_batch=VERIFIED)
        tapes = [hashlib.shake_256(b"registry-rate:tape:%d" % i).digest(api.tape_bytes(K)) for i in range(VERIFIED)]
        vpks, _, pis = ctx.verifiable_keygen(tapes)
        assert ctx.verify(pis, vpks) == [True] * VERIFIED
        ctx.registry_reserve(VERIFIED)
        slots = (C.c_int32 * VERIFIED)(*range(VERIFIED))
        done = C.create_string_buffer(VERIFIED)
        fn = lambda: lib.kosk_registry_admit_verified(ctx.handle, VERIFIED, slots, done)
        for _ in range(3):
            assert fn() == 0 and done.raw == b"\x01" * VERIFIED
        out["admit_verified %d" % VERIFIED] = [window(ctx, fn, VERIFIED, a.seconds) for _ in range(a.repeats)]
    ctx.close()
    print("RESULT " + json.dumps(out), flush=True)


def run_worker(a, mode, lib_path):
    env = dict(os.environ)
    env.pop("KOSK_LIB_PATH", None)
    if lib_path:
        env["KOSK_LIB_PATH"] = os.path.abspath(lib_path)
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--sizes", a.sizes, "--seconds", str(a.seconds), "--repeats", str(a.repeats)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    for ln in r.stdout.splitlines():
        if ln.startswith("RESULT "):
            return json.loads(ln[7:])
    raise SystemExit("worker %s failed (exit %d):\n%s" % (mode, r.returncode, r.stdout[-3000:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", help="the parent commit's libkosk_mi355x.so: the yardstick")
    ap.add_argument("--sizes", default="46,4096,65536")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    ap.add_argument("--worker", default="", choices=["", "old", "new", "slots"], help="(internal) measure in this process and print one JSON line")
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
    say("registry_rate: Kyber-768, %d distinct keys over and over; window >= %.1f s, %d repeats; items/s by stream events, device buffers" % (KEYS, a.seconds, a.repeats))
    old = run_worker(a, "old", a.parent_lib)
    new = run_worker(a, "new", None)
    slots = run_worker(a, "slots", None)
    sizes = [int(x) for x in a.sizes.split(",")]
    say("-- kosk_kem_enc_slots next to the per-item call on the same keys and the one-key call")
    below = 0
    for n in sizes:
        assert old["digest %d" % n] == new["digest %d" % n] == slots["digest %d" % n], "the legs disagree on ct / ss"
        y, t, k1 = old["enc_batch %d" % n], new["enc_batch %d" % n], new["enc_key %d" % n]
        for shape in ("distinct", "one"):
            s = slots["enc_slots %s %d" % (shape, n)]
            below += med(s) < med(y)
            say("enc n %6d  slots %-8s %s median %.0f | per-item: parent median %.0f (spread %.0f), tree median %.0f | one-key median %.0f | slots / per-item %.2f, slots / one-key %.2f"
                % (n, shape, " ".join("%.0f" % v for v in s), med(s), med(y), max(y) - min(y), med(t), med(k1), med(s) / med(y), med(s) / med(k1)))
    say("-- admissions (kosk_registry_admit, pk records in device memory, every call replaces the same n slots)")
    for n in sizes:
        s = slots["admit %d" % n]
        say("admit n %6d  %s median %.0f keys/s = %.1f us per call" % (n, " ".join("%.0f" % v for v in s), med(s), n / med(s) * 1e6))
    s = slots["admit_verified %d" % VERIFIED]
    say("admit_verified n %d  %s median %.0f keys/s = %.1f us per call" % (VERIFIED, " ".join("%.0f" % v for v in s), med(s), VERIFIED / med(s) * 1e6))
    say("kosk_kem_key_set (pk from host memory, wall clock): first %.0f us (allocates), then median %.0f us, min %.0f, max %.0f (20 loads)" % tuple(slots["key_set_us"]))
    say("launches of k_registry_admit %d, launch groups kem_enc_slots %d; ids 12 / 20 in that process: %d / %d" % tuple(slots["groups"]))
    say("-- the existing calls on the touched kernels: this tree against the parent's library (margin: the parent's max - min)")
    outside = 0
    for n in sizes:
        for what in ("enc_batch", "dec_batch", "enc_key", "dec_key"):
            y, t = old["%s %d" % (what, n)], new["%s %d" % (what, n)]
            spread = max(y) - min(y)
            ok = med(t) >= med(y) - spread
            outside += not ok
            say("%-9s n %6d  parent %s median %.0f (spread %.0f) | tree %s median %.0f  = %.3f  %s"
                % (what, n, " ".join("%.0f" % v for v in y), med(y), spread, " ".join("%.0f" % v for v in t), med(t), med(t) / med(y),
                   "inside" if ok else "BELOW the parent's margin"))
    say("result: kosk_kem_enc_slots is %s the per-item call at every size; %d of %d existing legs below the parent's margin"
        % ("above" if not below else "BELOW (%d shapes)" % below, outside, 4 * len(sizes)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
