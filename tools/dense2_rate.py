"""What the dense wire format kosk-dense-v2 buys against kosk-dense-v1 on the host-pointer calls, and whether v1 got slower by sharing its
templated body with v2.  The method of tools/dense_rate.py.

    python tools/dense2_rate.py [--k 3] [--sizes 46,736] [--rounds 5] [--parent-lib LIB] [--repeats 3] [--bench] [--out FILE]

1. v2 against v1, same tree, same session: per batch size n (one handle of max_batch n, one caller thread) and per kind of record buffer
   (pageable, page-locked from kosk_host_alloc) every round times one call each of kosk_verifiable_keygen_batch_dense, the same in v2
   (kosk_verifiable_keygen_batch_fmt, KOSK_FMT_DENSE2), kosk_verify_batch_dense and kosk_verify_batch_fmt (v2), in that order; medians
   over the rounds.  Then the refill alone between kosk_stream_timer_start / _stop: kosk_dense_fill_device against kosk_dense2_fill_device
   on the n resident images, alternated.
2. --parent-lib LIB (the parent commit's libkosk_mi355x.so): v1 alone on LIB and on this tree's library, each in a fresh child process
   (KOSK_LIB_PATH), alternated --repeats times.  The yardstick is the parent's library; its margin is its own max - min over the repeats.
3. --bench (with --parent-lib): bench.py at its defaults on LIB and on this tree, alternated --repeats times.
Parts 2 and 3 run first, before this process opens the GPU."""
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


def buffers(lib, mem, sizes, n):
    keep, ptrs = {}, {}
    for name, size in sizes.items():
        if mem == "pinned":
            ptrs[name] = lib.kosk_host_alloc(size * n)
            assert ptrs[name]
        else:
            keep[name] = C.create_string_buffer(size * n)
            ptrs[name] = C.addressof(keep[name])
    return keep, ptrs


def fill_alone(ctx, lib, torch, n, rounds, calls):
    """{name: [ms per round]} of the refill calls on the resident images, alternated inside every round"""
    d_img, stride = C.c_void_p(), C.c_size_t()
    assert lib.kosk_resident_proofs(ctx.handle, C.byref(d_img), C.byref(stride)) == 0
    d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ms = {name: [] for name in calls}
    for rnd in range(-1, rounds):
        for name, fn in calls.items():
            ctx.timer_start()
            fn(n, d_img.value, stride.value, d_st.data_ptr())
            t = ctx.timer_stop_ms()
            if rnd >= 0:
                ms[name].append(t)
    assert not d_st.any().item()
    return ms


def child_v1(args):
    """v1 alone on whatever library KOSK_LIB_PATH names: one JSON line {"n<n>_<mem>_<op>": median ms, "n<n>_fill": median ms}"""
    import torch
    from mpcith_kyber_kosk_amd import api
    from tests import oracle_lib
    lib, k = api.lib, args.k
    out = {}
    for n in [int(x) for x in args.sizes.split(",")]:
        ctx = api.Kosk(kyber_k=k, max_batch=n)
        h = ctx.handle
        tapes = b"".join(oracle_lib.tape_bytes_for(k, 5000 + b) for b in range(n))
        pk = C.create_string_buffer(ctx.pk_bytes * n); sk = C.create_string_buffer(ctx.sk_bytes * n); ok = C.create_string_buffer(n)
        for mem in ("pageable", "pinned"):
            keep, ptrs = buffers(lib, mem, {"dense": api.dense_proof_bytes(k)}, n)
            rec = C.c_void_p(ptrs["dense"])
            ops = {"keygen_batch_dense": lambda: lib.kosk_verifiable_keygen_batch_dense(h, n, tapes, ctx.tape_bytes, pk, sk, rec),
                   "verify_batch_dense": lambda: lib.kosk_verify_batch_dense(h, n, rec, pk, ok)}
            times = {name: [] for name in ops}
            for rnd in range(-1, args.rounds):
                for name, fn in ops.items():
                    t0 = time.perf_counter()
                    rc = fn()
                    dt = time.perf_counter() - t0
                    assert rc == 0 and (name != "verify_batch_dense" or ok.raw == b"\x01" * n), name
                    if rnd >= 0:
                        times[name].append(dt)
            for name in ops:
                out["n%d_%s_%s" % (n, mem, name)] = 1e3 * statistics.median(times[name])
            if mem == "pinned":
                lib.kosk_host_free(rec)
        ms = fill_alone(ctx, lib, torch, n, args.rounds, {"fill": ctx.dense_fill_device})
        out["n%d_fill" % n] = statistics.median(ms["fill"])
        ctx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--sizes", default="46,736")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--out", default="")
    ap.add_argument("--child-v1", action="store_true", help="(internal) measure v1 alone in this process and print one JSON line")
    args = ap.parse_args()
    if args.child_v1:
        return child_v1(args)
    if args.out:
        open(args.out, "w").close()

    def say(s):
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")

    def child(cmd, lib_path):
        env = dict(os.environ)
        env.pop("KOSK_LIB_PATH", None)
        if lib_path:
            env["KOSK_LIB_PATH"] = lib_path
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=500, env=env, cwd=ROOT)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
        if r.returncode != 0 or not lines:
            raise SystemExit("child failed (rc %d): %s" % (r.returncode, r.stderr[-400:]))
        return json.loads(lines[-1])

    if args.parent_lib:
        me = [sys.executable, os.path.abspath(__file__), "--child-v1", "--k", str(args.k), "--sizes", args.sizes, "--rounds", str(args.rounds)]
        runs = {"parent": [], "tree": []}
        for rep in range(args.repeats):
            for side in (("parent", "tree") if rep % 2 == 0 else ("tree", "parent")):
                runs[side].append(child(me, args.parent_lib if side == "parent" else ""))
        say("# v1 alone, the parent commit's library against this tree's, fresh child processes alternated %d times; ms, medians of %d rounds per child"
            % (args.repeats, args.rounds))
        say("# margin = the parent's own max - min over its repeats; 'slower' = this tree's median above the parent's median by more than that")
        for key in runs["parent"][0]:
            p = [r[key] for r in runs["parent"]]; t = [r[key] for r in runs["tree"]]
            margin = max(p) - min(p)
            verdict = "slower" if statistics.median(t) > statistics.median(p) + margin else "inside the margin" if statistics.median(t) >= statistics.median(p) - margin else "faster"
            say("%-36s parent %s  median %.3f  margin %.3f | tree %s  median %.3f | %s"
                % (key, " ".join("%.3f" % x for x in p), statistics.median(p), margin, " ".join("%.3f" % x for x in t), statistics.median(t), verdict))
        if args.bench:
            cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"]
            runs = {"parent": [], "tree": []}
            for rep in range(args.repeats):
                for side in (("parent", "tree") if rep % 2 == 0 else ("tree", "parent")):
                    runs[side].append(child(cmd, args.parent_lib if side == "parent" else "")["value"])
            say("# bench.py at its defaults (proofs/s), the parent's library and this tree alternated %d times" % args.repeats)
            for side in ("parent", "tree"):
                say("bench.py %-6s %s  median %.0f  min %.0f  max %.0f" % (side, " ".join("%.0f" % x for x in runs[side]), statistics.median(runs[side]),
                                                                          min(runs[side]), max(runs[side])))

    import torch
    from mpcith_kyber_kosk_amd import api
    from tests import oracle_lib
    if not torch.cuda.is_available():
        raise SystemExit("tools/dense2_rate.py needs a GPU")
    lib, k = api.lib, args.k
    ib, b1, b2 = api.proof_bytes(k), api.dense_proof_bytes(k), api.dense2_proof_bytes(k)
    say("# tools/dense2_rate.py: K = %d, record bytes image %d dense v1 %d (%.1f %%) dense v2 %d (%.1f %%; %.1f %% below v1), %d rounds, medians"
        % (k, ib, b1, 100.0 * b1 / ib, b2, 100.0 * b2 / ib, 100.0 * (b1 - b2) / b1, args.rounds))
    for n in [int(x) for x in args.sizes.split(",")]:
        ctx = api.Kosk(kyber_k=k, max_batch=n)
        h = ctx.handle
        tapes = b"".join(oracle_lib.tape_bytes_for(k, 5000 + b) for b in range(n))
        pk = C.create_string_buffer(ctx.pk_bytes * n); sk = C.create_string_buffer(ctx.sk_bytes * n); ok = C.create_string_buffer(n)
        ones = b"\x01" * n
        for mem in ("pageable", "pinned"):
            keep, ptrs = buffers(lib, mem, {"v1": b1, "v2": b2}, n)
            vp = {name: C.c_void_p(p) for name, p in ptrs.items()}
            ops = {
                "keygen_batch v1": lambda: lib.kosk_verifiable_keygen_batch_dense(h, n, tapes, ctx.tape_bytes, pk, sk, vp["v1"]),
                "keygen_batch v2": lambda: lib.kosk_verifiable_keygen_batch_fmt(h, api.FMT_DENSE2, n, tapes, ctx.tape_bytes, pk, sk, vp["v2"]),
                "verify_batch v1": lambda: lib.kosk_verify_batch_dense(h, n, vp["v1"], pk, ok),
                "verify_batch v2": lambda: lib.kosk_verify_batch_fmt(h, api.FMT_DENSE2, n, vp["v2"], pk, ok),
            }
            times = {name: [] for name in ops}
            for rnd in range(-1, args.rounds):  # round -1 fills the record buffers and warms up; it is not counted
                for name, fn in ops.items():
                    t0 = time.perf_counter()
                    rc = fn()
                    dt = time.perf_counter() - t0
                    if rc:
                        ctx._chk(rc, name)
                    if name.startswith("verify") and ok.raw != ones:
                        raise SystemExit("%s rejected an honest proof" % name)
                    if rnd >= 0:
                        times[name].append(dt)
            for op in ("verify_batch", "keygen_batch"):
                m1, m2 = statistics.median(times[op + " v1"]), statistics.median(times[op + " v2"])
                for name, med in ((op + " v1", m1), (op + " v2", m2)):
                    say("n %4d %-8s %-16s %9.1f proofs/s   median %8.3f ms   runs %s"
                        % (n, mem, name, n / med, 1e3 * med, " ".join("%.2f" % (1e3 * x) for x in times[name])))
                say("n %4d %-8s %-16s v2 / v1 time = %.3f (%s)" % (n, mem, op, m2 / m1, "v2 pays" if m2 < m1 else "v2 does NOT pay"))
            if mem == "pinned":
                for p in ptrs.values():
                    lib.kosk_host_free(C.c_void_p(p))
        ms = fill_alone(ctx, lib, torch, n, args.rounds, {"v1": ctx.dense_fill_device, "v2": ctx.dense2_fill_device})
        for name in ("v1", "v2"):
            med = statistics.median(ms[name])
            say("n %4d refill alone %s (setup + fill, stream timer): median %.3f ms per call = %.2f us per proof   runs %s"
                % (n, name, med, 1e3 * med / n, " ".join("%.3f" % x for x in ms[name])))
        say("n %4d refill alone v2 / v1 = %.3f" % (n, statistics.median(ms["v2"]) / statistics.median(ms["v1"])))
        ctx.close()


if __name__ == "__main__":
    main()
