"""Encapsulations/s and decapsulations/s of the KEM calls (kosk_kem_enc_batch / kosk_kem_dec_batch), Kyber-768.

    python tools/kem_rate.py [--sizes 46,4096,65536] [--seconds 1.0] [--repeats 3] [--out FILE]

Per n: public keys, coins, ciphertexts, secret keys and all outputs resident in HBM (torch tensors handed over as device pointers);
each shape is warmed up, then whole calls are counted inside a window of at least --seconds between two events on the handle's stream
(kosk_stream_timer_start / _stop; every call ends synchronised, so the window holds complete calls only), --repeats times.  n = 4096 is
also run with host buffers (everything crosses PCIe from and to pageable memory).  Every decapsulation's secrets are compared with the
encapsulation's once per shape.

Baseline, same command, same box: the reference's crypto_kem_enc_derand / crypto_kem_dec (kyber/kem.c, compiled into
oracle/_ref/libkyber_ref_k3.so by oracle/Makefile) called through ctypes on one core; skipped with a note where oracle/_ref is absent.
"""
import argparse
import ctypes as C
import hashlib
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, NKEYS = 3, 64


def window(ctx, call, n, seconds):
    """items/s over whole calls inside >= `seconds`, by the stream events; (rate by events, rate by wall clock, calls)"""
    calls = 0
    ctx.timer_start()
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        call()
        calls += 1
    wall = time.perf_counter() - t0
    ms = ctx.timer_stop_ms()
    return n * calls / (ms * 1e-3), n * calls / wall, calls


def reference_rates(keys, seconds):
    path = os.path.join(ROOT, "oracle", "_ref", "libkyber_ref_k%d.so" % K)
    if not os.path.exists(path):
        return None
    ref = C.CDLL(path)
    enc, dec = ref.pqcrystals_kyber768_ref_enc_derand, ref.pqcrystals_kyber768_ref_dec
    ct, ss, ss2 = C.create_string_buffer(1088), C.create_string_buffer(32), C.create_string_buffer(32)
    pk, sk = keys[0]
    m = hashlib.sha3_256(b"kem-rate").digest()
    out = []
    for fn in (lambda: enc(ct, ss, pk, m), lambda: dec(ss2, ct, sk)):
        for _ in range(200):
            fn()
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < seconds:
            for _ in range(100):
                fn()
            n += 100
        out.append(n / (time.perf_counter() - t0))
    assert ss.raw == ss2.raw
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="46,4096,65536")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from mpcith_kyber_kosk_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("tools/kem_rate.py needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    keys = [api.host_keygen(K, hashlib.shake_256(b"kem-rate:kg:%d" % i).digest(64))[:2] for i in range(NKEYS)]
    ctx = api.Kosk(kyber_k=K, max_batch=1)
    ctb = api.ct_bytes(K)
    dev = lambda blob: torch.frombuffer(bytearray(blob), dtype=torch.uint8).cuda()
    say("kem_rate: Kyber-768, %s, window >= %.1f s, %d repeats; items/s by stream events (by wall clock)" % (torch.cuda.get_device_name(0), a.seconds, a.repeats))
    med = {}
    for n in [int(x) for x in a.sizes.split(",")]:
        pks = [keys[b % NKEYS][0] for b in range(n)]; sks = [keys[b % NKEYS][1] for b in range(n)]
        coins = [hashlib.shake_256(b"kem-rate:m:%d" % b).digest(32) for b in range(n)]
        d_pk, d_sk, d_m = dev(b"".join(pks)), dev(b"".join(sks)), dev(b"".join(coins))
        d_ct = torch.empty(n * ctb, dtype=torch.uint8, device="cuda"); d_ss = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        d_ss2 = torch.empty(n * 32, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        shapes = [("device", lambda: ctx.kem_enc(d_pk.data_ptr(), d_m.data_ptr(), n=n, out=(d_ct.data_ptr(), d_ss.data_ptr())),
                   lambda: ctx.kem_dec(d_ct.data_ptr(), d_sk.data_ptr(), n=n, out=d_ss2.data_ptr()))]
        if n == 4096:
            pkb, skb, mb = b"".join(pks), b"".join(sks), b"".join(coins)
            h_ct, h_ss, h_ss2 = C.create_string_buffer(n * ctb), C.create_string_buffer(n * 32), C.create_string_buffer(n * 32)
            h = ctx.handle
            shapes.append(("host", lambda: api.lib.kosk_kem_enc_batch(h, n, pkb, mb, h_ct, h_ss), lambda: api.lib.kosk_kem_dec_batch(h, n, h_ct, skb, h_ss2)))
        for where, enc, dec in shapes:
            for _ in range(3):  # warm-up of this shape (the first call also allocates the KEM workspace)
                enc(); dec()
            if where == "device":
                assert torch.equal(d_ss, d_ss2), "dec(enc) != ss"
            else:
                assert h_ss.raw == h_ss2.raw
            for what, fn in (("enc", enc), ("dec", dec)):
                runs = [window(ctx, fn, n, a.seconds) for _ in range(a.repeats)]
                med[(what, where, n)] = statistics.median(r[0] for r in runs)
                say("%s n %6d %-6s buffers: %s /s   median %.0f   (%d calls per window)"
                    % (what, n, where, "  ".join("%.0f (%.0f)" % (r[0], r[1]) for r in runs), med[(what, where, n)], runs[0][2]))
        del d_pk, d_sk, d_m, d_ct, d_ss, d_ss2
    ref = reference_rates(keys, a.seconds)
    if ref is None:
        say("reference baseline: oracle/_ref absent, not measured")
    else:
        say("reference (kyber/kem.c, one core, through ctypes): enc_derand %.0f /s (%.1f us)   dec %.0f /s (%.1f us)" % (ref[0], 1e6 / ref[0], ref[1], 1e6 / ref[1]))
        for (what, where, n), v in sorted(med.items()):
            say("ratio %s n %6d %-6s: %.1f x one reference core" % (what, n, where, v / ref[0 if what == "enc" else 1]))
    pc = ctx.path_counts()
    say("launch groups: kem_enc %d kem_dec %d" % (pc["kem_enc"], pc["kem_dec"]))
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
