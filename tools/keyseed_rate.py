"""What deriving the proof randomness from the key (format kosk-keyseed-v1, k_keyseed) costs, Kyber-768, one handle (max_batch 736),
secret keys resident in HBM.

    python tools/keyseed_rate.py [--rounds 5] [--calls 20] [--out profiles/keyseed_rate.txt]

Staging, n = 46 and n = 736: kosk_stage_prover_keys_derived next to kosk_stage_prover_keys_seeded (seeds resident in HBM too), as
ALTERNATING calls A B A B ... after a warm-up of both; host clock around calls that end synchronised; `calls` calls per leg and round,
the round's figure is their mean, reported: the rounds and their median.  The ratio derived / seeded is the ratio of the medians.
Derivation alone: kosk_keyseed_device on the same resident records (read in place: one launch of k_keyseed and the call's
synchronisation, no copy), `calls` calls between the library's stream-timer events, unsalted and unbound, then armed-style with
contexts and salts resident in HBM.  Per permutation: the call's time over 19 (the chain one wave walks at K = 3; every key's wave
walks it at the same time).  The yardstick is the wave sponge's time per permutation inside the Fiat-Shamir chains
(profiles/r06_fs_device.txt).
"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
K, SIZES, PERMS = 3, (46, 736), 19


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    import torch
    from mpcith_kyber_kosk_amd import api
    if not torch.cuda.is_available():
        raise SystemExit("tools/keyseed_rate.py needs a GPU")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    big = max(SIZES)
    ctx = api.Kosk(kyber_k=K, max_batch=big)
    lib, h = api.lib, ctx.handle
    keys = [api.host_keygen(K, bytes([i + 1]) * 64)[1] for i in range(8)]
    d_sk = torch.frombuffer(bytearray(b"".join(keys[b % 8] for b in range(big))), dtype=torch.uint8).cuda()
    d_seed = torch.zeros((big * 32,), dtype=torch.uint8, device="cuda")
    d_cx = torch.arange(big * 32, dtype=torch.int32, device="cuda").to(torch.uint8)
    d_sa = torch.flip(d_cx, dims=[0]).contiguous()
    torch.cuda.synchronize()
    sk_p, seed_p = C.c_void_p(d_sk.data_ptr()), C.c_void_p(d_seed.data_ptr())
    okbuf = C.create_string_buffer(big)

    def must(rc, what):
        if rc:
            raise SystemExit(what + ": " + lib.kosk_last_error(h).decode())

    def derive_ms(n, calls, full):
        cx = C.c_void_p(d_cx.data_ptr()) if full else None
        sa = C.c_void_p(d_sa.data_ptr()) if full else None
        ctx.timer_start()
        for _ in range(calls):
            must(lib.kosk_keyseed_device(h, n, sk_p, cx, 32, sa, 32, seed_p), "kosk_keyseed_device")
        return ctx.timer_stop_ms() / calls

    def leg(fn, n, calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn(n)
        us = (time.perf_counter() - t0) * 1e6 / calls
        assert okbuf.raw[:n] == b"\x01" * n
        return us

    def derived(n):
        must(lib.kosk_stage_prover_keys_derived(h, n, sk_p, None, 0, okbuf), "kosk_stage_prover_keys_derived")

    def seeded(n):
        must(lib.kosk_stage_prover_keys_seeded(h, n, sk_p, seed_p, 32, okbuf), "kosk_stage_prover_keys_seeded")

    say("keyseed_rate: Kyber-768, %s, one handle (max_batch %d), %d rounds of %d calls per leg" % (torch.cuda.get_device_name(0), big, a.rounds, a.calls))
    for n in SIZES:
        derive_ms(n, 5, False); derive_ms(n, 5, True)
        for full, name in ((False, "unbound, unsalted"), (True, "contexts + salts in HBM")):
            runs = [derive_ms(n, a.calls, full) * 1e3 for _ in range(a.rounds)]
            med = statistics.median(runs)
            say("kosk_keyseed_device alone, n %3d, %-23s: %s us per call, median %.2f us = %.3f us per permutation (%d per key)"
                % (n, name, "  ".join("%.2f" % r for r in runs), med, med / PERMS, PERMS))
        # the seeds the seeded leg reads are the ones the derived leg makes: both legs leave the same tapes
        must(lib.kosk_keyseed_device(h, n, sk_p, None, 0, None, 0, seed_p), "kosk_keyseed_device")
        for _ in range(3):
            leg(derived, n, 2); leg(seeded, n, 2)
        A, B = [], []
        for _ in range(a.rounds):
            A.append(leg(derived, n, a.calls))
            B.append(leg(seeded, n, a.calls))
        ma, mb = statistics.median(A), statistics.median(B)
        say("kosk_stage_prover_keys_derived, n %3d: %s us per call, median %.1f" % (n, "  ".join("%.1f" % r for r in A), ma))
        say("kosk_stage_prover_keys_seeded,  n %3d: %s us per call, median %.1f" % (n, "  ".join("%.1f" % r for r in B), mb))
        say("derived / seeded, n %3d: %.3f (difference of the medians %+.1f us)" % (n, ma / mb, ma - mb))
    ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
