"""The needles of the erasure tests (tests/test_wipe_host.py, tests/test_gpu_24_wipe.py, tests/gpu_child_wipe.py):
byte strings that a call plants in the handle's memory and that must be gone after a wipe, and the calls that plant them.

Every needle is 32 bytes of high-entropy data -- outputs of SHAKE / SHA3 or of a binomial sampler's packed NTT -- except the first 32
coefficients of s, 64 bytes, in two forms: as int16 (what the sampler's output buffer holds) and as canonical u16 mod q (what a row of
the row matrix holds).  The control needle is public: bytes 0..31 of a pk.  Needle() refuses a run of one byte value: zeroed memory is
full of those."""
import hashlib

Q = 3329
KS = (2, 3)


class Needle:
    def __init__(self, name, data):
        data = bytes(data)
        assert len(data) in (32, 64), (name, len(data))
        assert len(set(data)) > 1, "needle %s is a run of one byte value" % name
        self.name, self.data = name, data

    def __repr__(self):
        return "Needle(%s)" % self.name


def tape(k, i):
    from tests import oracle_lib
    return oracle_lib.tape_bytes_for(k, 24000 + i)


def seed(i):
    return hashlib.sha3_256(b"kosk-wipe-v1:seed:%d" % i).digest()


def coins32(i):
    return hashlib.sha3_256(b"kosk-wipe-v1:m:%d" % i).digest()


def coins64(i):
    return hashlib.sha3_512(b"kosk-wipe-v1:dz:%d" % i).digest()


def context(i):
    return hashlib.sha3_256(b"kosk-wipe-v1:context:%d" % i).digest()


def tape_needles(t, key_seed=True):
    out = [Needle("tape: first PRF seed", t[64:96])]
    if key_seed:
        out.append(Needle("tape: key seed", t[0:32]))
    return out


def sk_needles(sk):
    return [Needle("sk: z", sk[-32:]), Needle("sk: packed NTT(s)", sk[:32])]


def s_needles(k, seed64):
    """the first 32 coefficients of s of host kosk_keygen on seed64, as int16 and as canonical u16"""
    import numpy as np
    from mpcith_kyber_kosk_amd import api
    s = np.array([int(x) for x in api.host_keygen(k, seed64)[3][:32]], dtype=np.int64)
    return [Needle("s: int16", s.astype("<i2").tobytes()), Needle("s: canonical u16", (s % Q).astype("<u2").tobytes())]


def honest_keys(k, n, first=0):
    """(pks, sks) of n honest key pairs that no call of the handle under test made"""
    from tests import keyproof_cases as kc
    ks = [kc.honest(k, first + i) for i in range(n)]
    return [x[0] for x in ks], [x[1] for x in ks]


# ---- the planting calls: fn(ctx) -> (needles, results); results are compared byte for byte between handles
def plant_keygen_tapes(ctx, n=2, first=0):
    tapes = [tape(ctx.k, first + b) for b in range(n)]
    res = ctx.verifiable_keygen(tapes)
    b = n - 1
    return tape_needles(tapes[b]) + sk_needles(res[1][b]) + s_needles(ctx.k, tapes[b][:64]), res


def plant_keygen_seeded(ctx, n=2, first=0):
    from mpcith_kyber_kosk_amd import api
    seeds = [seed(first + b) for b in range(n)]
    res = ctx.verifiable_keygen(seeds=seeds)
    b = n - 1
    t = api.tape_from_seed(ctx.k, seeds[b])
    return [Needle("seed of a seeded call", seeds[b])] + tape_needles(t) + sk_needles(res[1][b]), res


def plant_keygen_compact(ctx, n=2, first=10):
    tapes = [tape(ctx.k, first + b) for b in range(n)]
    res = ctx.verifiable_keygen_compact(tapes)
    return tape_needles(tapes[n - 1]) + sk_needles(res[1][n - 1]), res


def plant_keygen_dense(ctx, n=2, first=20):
    tapes = [tape(ctx.k, first + b) for b in range(n)]
    res = ctx.verifiable_keygen_dense(tapes)
    return tape_needles(tapes[n - 1]) + sk_needles(res[1][n - 1]), res


def plant_keygen_resident(ctx, n=2, first=30):
    tapes = [tape(ctx.k, first + b) for b in range(n)]
    ctx.verifiable_keygen_resident(tapes)
    pks, sks = ctx.keys(n)
    return tape_needles(tapes[n - 1]) + sk_needles(sks[n - 1]), (pks, sks, ctx.fetch_proofs(n))


def plant_prove_keys_tapes(ctx, n=2, first=40):
    _pks, sks = honest_keys(ctx.k, n)
    tapes = [tape(ctx.k, first + b) for b in range(n)]
    res = ctx.prove_keys(sks, tapes=tapes)
    return tape_needles(tapes[n - 1], key_seed=False) + sk_needles(sks[n - 1]), res


def plant_prove_keys_seeded(ctx, n=2, first=40):
    _pks, sks = honest_keys(ctx.k, n)
    seeds = [seed(first + b) for b in range(n)]
    res = ctx.prove_keys(sks, seeds=seeds)
    return [Needle("seed of a seeded call", seeds[n - 1])] + sk_needles(sks[n - 1]), res


def plant_prove_keys_derived(ctx, n=2):
    from mpcith_kyber_kosk_amd import api
    _pks, sks = honest_keys(ctx.k, n)
    res = ctx.prove_keys(sks, derived=True)
    d = api.keyseed_value(ctx.k, sks[n - 1])
    return [Needle("derived seed", d)] + tape_needles(api.tape_from_seed(ctx.k, d), key_seed=False) + sk_needles(sks[n - 1]), res


def stage_keys(ctx, n=2, first=50):
    """the staging half of plant_stage_prove_resident"""
    _pks, sks = honest_keys(ctx.k, n)
    tapes = [tape(ctx.k, first + b) for b in range(n)]
    ok = ctx.stage_prover_keys(sks, tapes=tapes)
    return tape_needles(tapes[n - 1], key_seed=False) + sk_needles(sks[n - 1]), ok


def plant_stage_prove_resident(ctx, n=2, first=50):
    needles, ok = stage_keys(ctx, n, first)
    ctx.prove_resident(n)
    return needles, (ok, ctx.fetch_proofs(n))


def plant_kem_enc(ctx, n=3):
    pks, _sks = honest_keys(ctx.k, n)
    m = [coins32(b) for b in range(n)]
    cts, sss = ctx.kem_enc(pks, coins=m)
    return [Needle("enc: m", m[n - 1]), Needle("enc: ss", sss[n - 1])], (cts, sss)


def plant_kem_dec(ctx, n=3):
    pks, sks = honest_keys(ctx.k, n)
    # ciphertexts from the library's own encapsulation on a second handle would need one; a wrong ciphertext decapsulates as well
    # (implicit rejection: ss = PRF(z, ct)) and plants the same kinds of bytes
    from mpcith_kyber_kosk_amd import api
    cts = [hashlib.shake_256(b"kosk-wipe-v1:ct:%d" % b).digest(api.ct_bytes(ctx.k)) for b in range(n)]
    sss = ctx.kem_dec(cts, sks)
    return [Needle("dec: ss", sss[n - 1])] + sk_needles(sks[n - 1]), sss


def plant_kem_keypair(ctx, n=3):
    c = [coins64(b) for b in range(n)]
    pks, sks = ctx.kem_keypair(coins=c)
    return [Needle("keypair: d", c[n - 1][:32]), Needle("keypair: z", c[n - 1][32:])] + sk_needles(sks[n - 1]), (pks, sks)


def plant_kem_check_sk(ctx, n=3):
    _pks, sks = honest_keys(ctx.k, n, first=3)
    return sk_needles(sks[n - 1]), ctx.kem_check_sk(sks)


def plant_prepare(ctx, n=2, first=60):
    # these two calls read their own draws from the start of the tape they are given (the reference's main.cpp order)
    tapes = [tape(ctx.k, first + b) for b in range(n)]
    return [Needle("prepare: first PRF seed", tapes[n - 1][0:32])], (ctx.prepare_randomness(tapes), ctx.prepare_range_proof(tapes))


def plant_keygen_seeded_resident(ctx, n=2, first=10):
    from mpcith_kyber_kosk_amd import api
    seeds = [seed(first + b) for b in range(n)]
    ctx.verifiable_keygen_resident(seeds=seeds)
    pks, sks = ctx.keys(n)
    t = api.tape_from_seed(ctx.k, seeds[n - 1])
    return [Needle("seed of a seeded call", seeds[n - 1])] + tape_needles(t) + sk_needles(sks[n - 1]), (pks, sks, ctx.fetch_proofs(n))


def plant_keygen_seeded_compact(ctx, n=2, first=14):
    from mpcith_kyber_kosk_amd import api
    seeds = [seed(first + b) for b in range(n)]
    res = ctx.verifiable_keygen_compact(seeds=seeds)
    t = api.tape_from_seed(ctx.k, seeds[n - 1])
    return [Needle("seed of a seeded call", seeds[n - 1])] + tape_needles(t) + sk_needles(res[1][n - 1]), res


def plant_keygen_seeded_dense(ctx, n=2, first=18):
    from mpcith_kyber_kosk_amd import api
    seeds = [seed(first + b) for b in range(n)]
    res = ctx.verifiable_keygen_dense(seeds=seeds)
    t = api.tape_from_seed(ctx.k, seeds[n - 1])
    return [Needle("seed of a seeded call", seeds[n - 1])] + tape_needles(t) + sk_needles(res[1][n - 1]), res


def plant_prove_prepared(ctx, n=2, first=120):
    """kosk_prove_prepared on the outputs of kosk_prepare_* and the instances of host kosk_keygen (the split of one keygen tape,
    tests/test_gpu_03_split_api.py): the needles are the first 32 values of f_0 in the randomness record (a row of the row matrix), the
    first 32 coefficients of the instance's s in both forms, and the first bytes of the tape's online part"""
    import numpy as np
    from mpcith_kyber_kosk_amd import api
    from tests import oracle_lib
    k = ctx.k
    p = oracle_lib.params(k)
    a = 64 + 32 * p.M + 2 * p.M * 302
    b = a + 2 * k * p.E * 302
    tapes = [tape(k, first + i) for i in range(n)]
    rands = ctx.prepare_randomness([t[64:a] for t in tapes])
    rngs = ctx.prepare_range_proof([t[a:b] for t in tapes])
    insts = []
    for t in tapes:
        _pk, _sk, A, s, e, tt = api.host_keygen(k, t[:64])
        insts.append(b"".join(np.asarray(x, np.int16).tobytes() for x in (A, tt, s, e)))
    pis = ctx.prove_prepared(insts, rands, rngs, [t[b:] for t in tapes])
    last = tapes[n - 1]
    needles = [Needle("randomness: f_0", rands[n - 1][:64]), Needle("tape: online part", last[b:b + 32])] + s_needles(k, last[:64])
    return needles, (rands, rngs, pis)


def plant_kem_enc_verified(ctx, n=2, first=130):
    tapes = [tape(ctx.k, first + b) for b in range(n)]
    ctx.verifiable_keygen_resident(tapes)
    ok = ctx.verify_resident_pk(n)
    m = [coins32(40 + b) for b in range(n)]
    cts, sss, done = ctx.kem_enc_verified(n, coins=m)
    assert ok == [True] * n and done == [True] * n
    return [Needle("enc_verified: m", m[n - 1]), Needle("enc_verified: ss", sss[n - 1])], (cts, sss, done)


# the calls of test case 1 (mode off: the scan finds what each of them planted)
GROUND_TRUTH = [plant_keygen_tapes, plant_keygen_seeded, plant_prove_keys_derived, plant_stage_prove_resident, plant_kem_enc, plant_kem_dec,
                plant_kem_keypair, plant_kem_check_sk]
# the entry points that end with the wipe under WIPE_CALL and take host buffers only (the device-pointer ones are in the GPU test itself)
WIPE_CALL_PLANTS = GROUND_TRUTH + [plant_keygen_compact, plant_keygen_dense, plant_keygen_resident, plant_prove_keys_tapes,
                                   plant_prove_keys_seeded, plant_prepare, plant_prove_prepared, plant_kem_enc_verified,
                                   plant_keygen_seeded_resident, plant_keygen_seeded_compact, plant_keygen_seeded_dense]


def control(pk):
    return Needle("control: pk", pk[:32])
