"""Items/s of the one-key KEM calls (kosk_kem_enc_key / kosk_kem_dec_key) next to the per-item calls (kosk_kem_enc_batch /
kosk_kem_dec_batch) with the key replicated, Kyber-768, and the time of kosk_kem_key_set.

    python tools/kem_onekey_rate.py --parent-lib <the parent commit's libkosk_mi355x.so> [--sizes 46,4096,65536] [--seconds 1.0]
                                    [--repeats 3] [--out profiles/kem_onekey_rate.txt]

The method of tools/kem_rate.py: every buffer resident in HBM (torch tensors handed over as device pointers), each shape warmed up, then
whole calls counted inside a window of at least --seconds between two events on the handle's stream, --repeats times, median.  n = 4096
is also run from pageable host buffers.  The replicated-key figures come from the PARENT commit's library (KOSK_LIB_PATH), measured by
this same command: each library runs in a fresh child process of this one (`--worker`), one after the other.  The margin of the
comparison is the yardstick's own run-to-run spread, max - min of its repeats at that size.
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


def window(ctx, call, n, seconds):
    calls = 0
    ctx.timer_start()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        call()
        calls += 1
    return n * calls / (ctx.timer_stop_ms() * 1e-3)


def worker(a):
    """one library, one process: {"what where n": [rates]} as one JSON line; mode `batch` the per-item calls, `key` the one-key calls"""
    import torch
    from mpcith_kyber_kosk_amd import api
    pk, sk = api.host_keygen(K, hashlib.shake_256(b"kem-onekey-rate:kg").digest(64))[:2]
    ctx = api.Kosk(kyber_k=K, max_batch=1)
    lib, h, ctb = api.lib, ctx.handle, api.ct_bytes(K)
    dev = lambda blob: torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    out = {}
    if a.worker == "key":
        t = []
        for _ in range(21):
            t0 = time.perf_counter()
            ctx.kem_key_set(sk=sk)
            t.append((time.perf_counter() - t0) * 1e6)
        out["key_set_us"] = [t[0], statistics.median(t[1:]), min(t[1:]), max(t[1:])]
    for n in [int(x) for x in a.sizes.split(",")]:
        coins = b"".join(hashlib.shake_256(b"kem-onekey-rate:m:%d" % b).digest(32) for b in range(n))
        d_m = dev(coins)
        d_ct = torch.empty(n * ctb, dtype=torch.uint8, device="cuda"); d_ss = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        d_ss2 = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        h_ct, h_ss, h_ss2 = C.create_string_buffer(n * ctb), C.create_string_buffer(n * 32), C.create_string_buffer(n * 32)
        p = lambda t_: C.c_void_p(t_.data_ptr())
        if a.worker == "key":
            shapes = [("device", lambda: lib.kosk_kem_enc_key(h, n, p(d_m), p(d_ct), p(d_ss)), lambda: lib.kosk_kem_dec_key(h, n, p(d_ct), p(d_ss2)))]
            if n == 4096:
                shapes.append(("host", lambda: lib.kosk_kem_enc_key(h, n, coins, h_ct, h_ss), lambda: lib.kosk_kem_dec_key(h, n, h_ct, h_ss2)))
        else:
            pks, sks = pk * n, sk * n  # the key replicated: what a one-key party hands the per-item calls
            d_pk, d_sk = dev(pks), dev(sks)
            shapes = [("device", lambda: lib.kosk_kem_enc_batch(h, n, p(d_pk), p(d_m), p(d_ct), p(d_ss)),
                       lambda: lib.kosk_kem_dec_batch(h, n, p(d_ct), p(d_sk), p(d_ss2)))]
            if n == 4096:
                shapes.append(("host", lambda: lib.kosk_kem_enc_batch(h, n, pks, coins, h_ct, h_ss), lambda: lib.kosk_kem_dec_batch(h, n, h_ct, sks, h_ss2)))
        torch.cuda.synchronize()
        for where, enc, dec in shapes:
            for _ in range(3):
                assert enc() == 0 and dec() == 0
            if where == "device":
                assert torch.equal(d_ss, d_ss2), "dec(enc) != ss"
                out["digest %d" % n] = hashlib.sha3_256(bytes(d_ct.cpu().numpy()) + bytes(d_ss.cpu().numpy())).hexdigest()
            else:
                assert h_ss.raw == h_ss2.raw
            for what, fn in (("enc", enc), ("dec", dec)):
                out["%s %s %d" % (what, where, n)] = [window(ctx, fn, n, a.seconds) for _ in range(a.repeats)]
    if a.worker == "key":
        out["groups"] = [ctx.path_count(api.Kosk.PATH_KEM_KEY_SETUP), ctx.path_count(api.Kosk.PATH_KEM_ENC_KEY), ctx.path_count(api.Kosk.PATH_KEM_DEC_KEY)]
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
    ap.add_argument("--worker", default="", choices=["", "batch", "key"], help="(internal) measure in this process and print one JSON line")
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    if not a.parent_lib or not os.path.exists(a.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's library is the yardstick of this tool")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("kem_onekey_rate: Kyber-768, one key; window >= %.1f s, %d repeats; items/s by stream events" % (a.seconds, a.repeats))
    say("yardstick: kosk_kem_enc_batch / kosk_kem_dec_batch of the parent commit's library, the key replicated n times; then this tree")
    parent = run_worker(a, "batch", a.parent_lib)
    tree_batch = run_worker(a, "batch", None)
    key = run_worker(a, "key", None)
    slower = 0
    for n in [int(x) for x in a.sizes.split(",")]:
        assert parent["digest %d" % n] == tree_batch["digest %d" % n] == key["digest %d" % n], "the three legs disagree on ct / ss"
        for where in ("device", "host") if n == 4096 else ("device",):
            for what in ("enc", "dec"):
                name = "%s %s %d" % (what, where, n)
                y, t, o = parent[name], tree_batch[name], key[name]
                spread = max(y) - min(y)
                ok = statistics.median(o) >= statistics.median(y) - spread
                slower += not ok
                say("%s n %6d %-6s  parent per-item %s median %.0f (spread %.0f) | tree per-item median %.0f | one-key %s median %.0f  = %.2f x  %s"
                    % (what, n, where, " ".join("%.0f" % v for v in y), statistics.median(y), spread, statistics.median(t),
                       " ".join("%.0f" % v for v in o), statistics.median(o), statistics.median(o) / statistics.median(y),
                       "ok" if ok else "SLOWER than the yardstick beyond its spread"))
    ks = key["key_set_us"]
    say("kosk_kem_key_set (sk from host memory, wall clock): first %.0f us (allocates), then median %.0f us, min %.0f, max %.0f (20 loads, each replacing the slot)"
        % tuple(ks))
    say("launches of k_kem_key_setup %d, launch groups kem_enc_key %d kem_dec_key %d; ct / ss of the three legs are equal at every size" % tuple(key["groups"]))
    say("result: %s" % ("every one-key figure is at or above the yardstick" if not slower else "%d one-key figures are below the yardstick's spread" % slower))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
