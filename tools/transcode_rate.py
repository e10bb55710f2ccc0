"""What the GPU transcoder (kosk_transcode_batch) does per second next to the host codecs, and what the codeword
check costs next to the refill it shares its engine with; legs alternated in one session on one handle.

    python tools/transcode_rate.py [--k 3] [--sizes 46,736] [--rounds 5] [--host-records 4] [--out FILE]

Per batch size n (one handle of max_batch n, one caller thread; the records are n honest proofs of that handle):
  - the check alone: kosk_dense_check_device and, next to it in every round, kosk_dense_fill_device on the same n resident images,
    each between kosk_stream_timer_start / _stop (k_dense_setup + k_dense_check / k_dense_fill); both times and their ratio;
  - the calls: image -> dense and dense -> image, records in pageable memory and in kosk_host_alloc memory, wall clock of the call,
    records per second; the results are compared with each other (dense -> image of image -> dense is the input);
  - the host codecs kosk_proof_dense_pack / kosk_proof_dense_unpack on a handful of the same records on one core, and the ratio.
Medians over the rounds; round -1 warms up and is not counted.
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
    ap.add_argument("--host-records", type=int, default=4)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    from mpcith_kyber_kosk_amd import api
    from tests import oracle_lib
    if not torch.cuda.is_available():
        raise SystemExit("tools/transcode_rate.py needs a GPU")
    lib, k = api.lib, args.k
    if args.out:
        open(args.out, "w").close()

    def say(s):
        print(s, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(s + "\n")
    ib, db = api.format_bytes(k, api.FMT_IMAGE), api.format_bytes(k, api.FMT_DENSE)
    say("# tools/transcode_rate.py: K = %d, record bytes image %d dense %d (%.1f %%), %d rounds, medians" % (k, ib, db, 100.0 * db / ib, args.rounds))
    runs = lambda xs, scale=1e3: " ".join("%.3f" % (scale * x) for x in xs)
    for n in [int(x) for x in args.sizes.split(",")]:
        ctx = api.Kosk(kyber_k=k, max_batch=n)
        h = ctx.handle
        tapes = b"".join(oracle_lib.tape_bytes_for(k, 5000 + b) for b in range(n))
        pk = C.create_string_buffer(ctx.pk_bytes * n); sk = C.create_string_buffer(ctx.sk_bytes * n)
        images = C.create_string_buffer(ib * n)
        assert lib.kosk_verifiable_keygen_batch(h, n, tapes, ctx.tape_bytes, pk, sk, images) == 0
        # ---- the check next to the fill, on the resident images (the fill writes what is there already)
        d_img, stride = C.c_void_p(), C.c_size_t()
        assert lib.kosk_resident_proofs(h, C.byref(d_img), C.byref(stride)) == 0
        d_st = torch.full((2 * n,), 7, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        check, fill = [], []
        for rnd in range(-1, args.rounds):
            ctx.timer_start()
            ctx.dense_check_device(n, d_img.value, stride.value, d_st.data_ptr())
            t_check = ctx.timer_stop_ms()
            ctx.timer_start()
            ctx.dense_fill_device(n, d_img.value, stride.value, d_st.data_ptr() + 4 * n)
            t_fill = ctx.timer_stop_ms()
            if rnd >= 0:
                check.append(t_check); fill.append(t_fill)
        assert not d_st.any().item(), "an honest proof is not a codeword"
        mc, mf = statistics.median(check), statistics.median(fill)
        say("n %4d check alone (k_dense_setup + k_dense_check, stream timer): median %.3f ms = %.2f us per proof   runs %s" % (n, mc, 1e3 * mc / n, runs(check, 1)))
        say("n %4d fill  alone (k_dense_setup + k_dense_fill,  stream timer): median %.3f ms = %.2f us per proof   runs %s" % (n, mf, 1e3 * mf / n, runs(fill, 1)))
        say("n %4d check / fill = %.3f   (the fill's own spread: %.3f .. %.3f of its median)" % (n, mc / mf, min(fill) / mf, max(fill) / mf))
        # ---- the calls
        status = (C.c_int32 * n)()
        per_mem = {}
        for mem in ("pageable", "pinned"):
            bufs, ptrs = {}, {}
            for name, size in (("image", ib), ("dense", db), ("back", ib)):
                if mem == "pinned":
                    ptrs[name] = lib.kosk_host_alloc(size * n)
                    assert ptrs[name]
                else:
                    bufs[name] = C.create_string_buffer(size * n)
                    ptrs[name] = C.addressof(bufs[name])
            C.memmove(ptrs["image"], images, ib * n)
            vp = {name: C.c_void_p(p) for name, p in ptrs.items()}
            ops = {"image->dense": lambda: lib.kosk_transcode_batch(h, n, api.FMT_IMAGE, vp["image"], api.FMT_DENSE, vp["dense"], status),
                   "dense->image": lambda: lib.kosk_transcode_batch(h, n, api.FMT_DENSE, vp["dense"], api.FMT_IMAGE, vp["back"], status)}
            times = {name: [] for name in ops}
            for rnd in range(-1, args.rounds):
                for name in ("image->dense", "dense->image"):
                    t0 = time.perf_counter()
                    rc = ops[name]()
                    dt = time.perf_counter() - t0
                    if rc:
                        ctx._chk(rc, name)
                    if any(status):
                        raise SystemExit("%s: a nonzero status for an honest proof" % name)
                    if rnd >= 0:
                        times[name].append(dt)
            assert C.string_at(ptrs["back"], ib * n) == images.raw, "dense -> image of image -> dense is not the input"
            for name in ops:
                med = statistics.median(times[name])
                per_mem[mem, name] = n / med
                say("n %4d %-8s %-13s %10.1f records/s   median %8.3f ms   runs %s" % (n, mem, name, n / med, 1e3 * med, runs(times[name])))
            if mem == "pageable":
                dense0 = C.string_at(ptrs["dense"], db * n)
            if mem == "pinned":
                assert C.string_at(ptrs["dense"], db * n) == dense0
                for p in ptrs.values():
                    lib.kosk_host_free(C.c_void_p(p))
        # ---- the host codecs on one core
        m = min(args.host_records, n)
        pack, unpack = [], []
        for b in range(m):
            img = images.raw[b * ib:(b + 1) * ib]
            t0 = time.perf_counter(); rc, rec = api.dense_pack(k, img); pack.append(time.perf_counter() - t0)
            assert rc == 0 and rec == dense0[b * db:(b + 1) * db], "the host codec and the GPU disagree"
            t0 = time.perf_counter(); st, back = api.dense_unpack(k, rec); unpack.append(time.perf_counter() - t0)
            assert st == 0 and back == img
        hp, hu = statistics.median(pack), statistics.median(unpack)
        say("n %4d host codec, one core, %d records: kosk_proof_dense_pack %.1f ms = %.1f records/s, kosk_proof_dense_unpack %.1f ms = %.1f records/s"
            % (n, m, 1e3 * hp, 1 / hp, 1e3 * hu, 1 / hu))
        for mem in ("pageable", "pinned"):
            say("n %4d %-8s GPU / host codec: image->dense %.0fx, dense->image %.0fx" % (n, mem, per_mem[mem, "image->dense"] * hp, per_mem[mem, "dense->image"] * hu))
        say("n %4d launches of k_dense_check %d, refills %d" % (n, ctx.path_count(api.Kosk.PATH_DENSE_CHECK), ctx.path_count(api.Kosk.PATH_DENSE_FILL)))
        ctx.close()


if __name__ == "__main__":
    main()
