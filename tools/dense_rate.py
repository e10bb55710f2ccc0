"""What the dense wire format kosk-dense-v1 buys on the host-pointer calls: proofs/s of the image, compact and dense forms of the
verifier and of key generation + proving, alternated in one session on one handle.

    python tools/dense_rate.py [--k 3] [--sizes 46,736] [--rounds 5] [--out FILE]

Per batch size n (one handle of max_batch n, one caller thread) and per kind of record buffer (pageable, page-locked from
kosk_host_alloc) every round times one call each of kosk_verify_batch, kosk_verify_batch_compact, kosk_verify_batch_dense,
kosk_verifiable_keygen_batch_compact and kosk_verifiable_keygen_batch_dense, in that order; the medians over the rounds are reported.
Then, on the same handle:
  - the refill alone: kosk_dense_fill_device on the n resident images between kosk_stream_timer_start / _stop (k_dense_setup + k_dense_fill);
  - the copy rate of the compact staging call (kosk_stage_verifier_inputs_compact: H2D copy + unpack + pk decode, through the
    library's staging buffer), and from it the H2D time of the bytes the dense form saves against the compact one.
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=3)
    ap.add_argument("--sizes", default="46,736")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from mpcith_kyber_kosk_amd import api
    from tests import oracle_lib
    if not torch.cuda.is_available():
        raise SystemExit("tools/dense_rate.py needs a GPU")
    lib, k = api.lib, args.k
    if args.out:
        open(args.out, "w").close()

    def say(s):
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")
    ib, cb, db = api.proof_bytes(k), lib.kosk_compact_proof_bytes(k), api.dense_proof_bytes(k)
    say("# tools/dense_rate.py: K = %d, record bytes image %d compact %d (%.1f %%) dense %d (%.1f %%), %d rounds, medians"
        % (k, ib, cb, 100.0 * cb / ib, db, 100.0 * db / ib, args.rounds))
    for n in [int(x) for x in args.sizes.split(",")]:
        ctx = api.Kosk(kyber_k=k, max_batch=n)
        h = ctx.handle
        tapes = b"".join(oracle_lib.tape_bytes_for(k, 5000 + b) for b in range(n))
        pk = C.create_string_buffer(ctx.pk_bytes * n); sk = C.create_string_buffer(ctx.sk_bytes * n); ok = C.create_string_buffer(n)
        ones = b"\x01" * n
        sizes = {"image": ib, "compact": cb, "dense": db}
        for mem in ("pageable", "pinned"):
            bufs, ptrs = {}, {}
            for name, size in sizes.items():
                if mem == "pinned":
                    ptrs[name] = lib.kosk_host_alloc(size * n)
                    assert ptrs[name]
                else:
                    bufs[name] = C.create_string_buffer(size * n)
                    ptrs[name] = C.addressof(bufs[name])
            vp = {name: C.c_void_p(p) for name, p in ptrs.items()}
            assert lib.kosk_verifiable_keygen_batch(h, n, tapes, ctx.tape_bytes, pk, sk, vp["image"]) == 0
            ops = {
                "verify_batch": lambda: lib.kosk_verify_batch(h, n, vp["image"], pk, ok),
                "verify_batch_compact": lambda: lib.kosk_verify_batch_compact(h, n, vp["compact"], pk, ok),
                "verify_batch_dense": lambda: lib.kosk_verify_batch_dense(h, n, vp["dense"], pk, ok),
                "keygen_batch_compact": lambda: lib.kosk_verifiable_keygen_batch_compact(h, n, tapes, ctx.tape_bytes, pk, sk, vp["compact"]),
                "keygen_batch_dense": lambda: lib.kosk_verifiable_keygen_batch_dense(h, n, tapes, ctx.tape_bytes, pk, sk, vp["dense"]),
            }
            times = {name: [] for name in ops}
            for rnd in range(-1, args.rounds):  # round -1 fills the record buffers and warms up; it is not counted
                for name in ("keygen_batch_compact", "keygen_batch_dense", "verify_batch", "verify_batch_compact", "verify_batch_dense"):
                    t0 = time.perf_counter()
                    rc = ops[name]()
                    dt = time.perf_counter() - t0
                    if rc:
                        ctx._chk(rc, name)
                    if name.startswith("verify") and ok.raw != ones:
                        raise SystemExit("%s rejected an honest proof" % name)
                    if rnd >= 0:
                        times[name].append(dt)
            for name in ("verify_batch", "verify_batch_compact", "verify_batch_dense", "keygen_batch_compact", "keygen_batch_dense"):
                med = statistics.median(times[name])
                say("n %4d %-8s %-22s %9.1f proofs/s   median %8.3f ms   runs %s"
                    % (n, mem, name, n / med, 1e3 * med, " ".join("%.2f" % (1e3 * x) for x in times[name])))
            if mem == "pageable":
                # the refill alone, on the images the last dense verify left resident (refilling them again changes nothing)
                d_img, stride = C.c_void_p(), C.c_size_t()
                assert lib.kosk_resident_proofs(h, C.byref(d_img), C.byref(stride)) == 0
                d_st = torch.zeros(n, dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                fill = []
                for rnd in range(args.rounds + 1):
                    ctx.timer_start()
                    ctx.dense_fill_device(n, d_img.value, stride.value, d_st.data_ptr())
                    fill.append(ctx.timer_stop_ms())
                assert not d_st.any().item()
                fill_ms = statistics.median(fill[1:])
                stage = []
                for rnd in range(args.rounds + 1):
                    t0 = time.perf_counter()
                    assert lib.kosk_stage_verifier_inputs_compact(h, n, vp["compact"], pk) == 0
                    stage.append(time.perf_counter() - t0)
                stage_s = statistics.median(stage[1:])
                rate = n * cb / stage_s
                saved_ms = 1e3 * n * (cb - db) / rate
                say("n %4d refill alone (k_dense_setup + k_dense_fill, stream timer): median %.3f ms per call = %.2f us per proof   runs %s"
                    % (n, fill_ms, 1e3 * fill_ms / n, " ".join("%.3f" % x for x in fill[1:])))
                say("n %4d compact staging call: median %.3f ms for %.1f MB = %.2f GB/s; the %.1f MB the dense form saves are %.3f ms at that rate: refill / saved = %.2f"
                    % (n, 1e3 * stage_s, n * cb / 1e6, rate / 1e9, n * (cb - db) / 1e6, saved_ms, fill_ms / saved_ms))
            if mem == "pinned":
                for p in ptrs.values():
                    lib.kosk_host_free(C.c_void_p(p))
        ctx.close()


if __name__ == "__main__":
    main()
