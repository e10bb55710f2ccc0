"""GPU tests of kosk_kem_keypair_batch, kosk_kem_check_pk and kosk_kem_check_sk.  Expected key pairs come from
tests/golden/kem_keypair_v1.json (what the reference's crypto_kem_keypair_derand returned) and from the model of
tests/kem_keypair_cases.py (api.host_keygen with z in the last 32 bytes), which runs nothing of these calls; expected flags from that
file's 12-bit decode and hashlib.  Every comparison is exact and covers every item of every batch.  tests/test_kem_keypair_host.py runs
the device functions built for the host against the same fixture: where that passes and a test here fails, the fault is in how the
kernels deal out the work or in the host code, not in kosk_kem_dev.hpp."""
import pytest

from tests import kem_edges as ke
from tests import kem_fixture as kf
from tests import kem_keypair_cases as kk

pytestmark = pytest.mark.gpu

KS = kk.KS
CHUNK = 16384        # KEM_CHUNK of csrc/kosk_ctx.hpp: items per launch group
WAVE_MAX = 1024      # KEM_WAVE_MAX: up to here H(pk) runs one wave per item, above it one lane per item in k_kem_hpk
SENTINEL = 0xA5
POSITIONS = (0, 63, 64, 129)
Q = kk.Q


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return torch


@pytest.fixture(scope="module")
def handles(torch_cuda):
    from mpcith_kyber_kosk_amd import api
    hs = {k: api.Kosk(kyber_k=k, max_batch=3) for k in KS}
    yield hs
    for h in hs.values():
        h.close()


@pytest.fixture(scope="module")
def keys():
    """per K: coins and the model's key pairs of the 130 fixture items, checked against the fixture's digests -- computed once"""
    out = {}
    for k in KS:
        fx = kk.load()["k"]["k%d" % k]
        pairs = [kk.keypair(k, i) for i in range(kk.ITEMS)]
        for (pk, sk), rec in zip(pairs, fx["items"]):
            assert kk.sha3(pk) == rec["pk"] and kk.sha3(sk) == rec["sk"]
        out[k] = {"coins": [kk.coins(k, i) for i in range(kk.ITEMS)], "pk": [p for p, _ in pairs], "sk": [s for _, s in pairs], "fx": fx}
    return out


def _same(k, n, b, what, got, want):
    if got != want:
        at = next((j for j in range(min(len(got), len(want))) if got[j] != want[j]), min(len(got), len(want)))
        pytest.fail("K=%d n=%d position %d: first differing %s byte %d of %d / %d" % (k, n, b, what, at, len(got), len(want)))


def _keypairs_by_position(ctx, k, v, n):
    idx = [b % kk.ITEMS for b in range(n)]
    pks, sks = ctx.kem_keypair([v["coins"][i] for i in idx])
    assert len(pks) == len(sks) == n
    for b, i in enumerate(idx):
        _same(k, n, b, "pk", pks[b], v["pk"][i])
        _same(k, n, b, "sk", sks[b], v["sk"][i])
    return pks, sks


# ------------------------------------------------------------------------------------------------------ key generation --
@pytest.mark.parametrize("k", KS)
def test_fixture_in_one_call_and_alone(k, handles, keys):
    """all 130 fixture items in one call (every role of k_kem_kg_hash spans three waves; the items whose matrix needs a fourth SHAKE128
    block sit among them), then item 0 and one four-block item alone: the fixture's digests and the model, byte for byte"""
    ctx, v = handles[k], keys[k]
    pks, sks = _keypairs_by_position(ctx, k, v, kk.ITEMS)
    for i, rec in enumerate(v["fx"]["items"]):
        assert kk.sha3(pks[i]) == rec["pk"] and kk.sha3(sks[i]) == rec["sk"], (k, i)
    assert v["fx"]["four_block"]
    for i in (0, v["fx"]["four_block"][0]):
        (pk,), (sk,) = ctx.kem_keypair([v["coins"][i]])
        assert kk.sha3(pk) == v["fx"]["items"][i]["pk"] and kk.sha3(sk) == v["fx"]["items"][i]["sk"], (k, i)
        assert (pk, sk) == (v["pk"][i], v["sk"][i])


@pytest.mark.parametrize("n", (WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1, 17 * 64 - 1))
@pytest.mark.parametrize("k", KS)
def test_sizes_around_the_wave_sponge_limit(k, n, handles, keys):
    """in process, without KOSK_DEBUG_KEM_WAVE_MAX: the last two sizes at which H(pk) runs on the wave sponge and the first of the
    per-lane layout; above the limit n is no multiple of 64, so waves of k_kem_kg_hash straddle two roles"""
    _keypairs_by_position(handles[k], k, keys[k], n)


def test_per_lane_hpk_on_small_batches(torch_cuda, gpu_child):
    out = gpu_child("from tests.gpu_child_keypair import per_lane_hpk_on_small_batches as f; f(2); f(3); f(4)",
                    env={"KOSK_DEBUG_KEM_WAVE_MAX": "0"})
    for k in KS:
        assert "per_lane_hpk_on_small_batches ok %d" % k in out


def test_device_buffers_across_a_launch_group(handles, keys, torch_cuda):
    """K = 2, n = KEM_CHUNK + 3: coins and both outputs device buffers, so the second launch group works at `pointer + first * size`;
    a sentinel margin around both outputs; counter 15 counts the two launch groups"""
    from mpcith_kyber_kosk_amd import api
    torch = torch_cuda
    k, n, pad = 2, CHUNK + 3, 64
    ctx, v = handles[k], keys[k]
    pkb, skb = ctx.pk_bytes, ctx.sk_bytes
    idx = [b % kk.ITEMS for b in range(n)]
    d_coins = torch.frombuffer(bytearray(b"".join(v["coins"][i] for i in idx)), dtype=torch.uint8).cuda()
    d_pk = torch.full((pad + n * pkb + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_sk = torch.full((pad + n * skb + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = ctx.path_count(api.Kosk.PATH_KEM_KEYPAIR)
    ctx.kem_keypair(d_coins.data_ptr(), n=n, out=(d_pk.data_ptr() + pad, d_sk.data_ptr() + pad))
    assert ctx.path_count(api.Kosk.PATH_KEM_KEYPAIR) == before + 2
    pk, sk = bytes(d_pk.cpu().numpy()), bytes(d_sk.cpu().numpy())
    for buf in (pk, sk):
        assert buf[:pad] == bytes([SENTINEL]) * pad and buf[-pad:] == bytes([SENTINEL]) * pad
    for b, i in enumerate(idx):
        _same(k, n, b, "pk", pk[pad + b * pkb:pad + (b + 1) * pkb], v["pk"][i])
        _same(k, n, b, "sk", sk[pad + b * skb:pad + (b + 1) * skb], v["sk"][i])


def test_entropy(handles, keys):
    """coins=None: a randombytes callback sees exactly n calls of 64 bytes, in item order, and the keys are the model's on those
    bytes; without a callback two calls differ and every key passes kem_check_sk"""
    k, n = 3, 70
    ctx = handles[k]
    seen = []

    def rb(nbytes):
        seen.append(nbytes)
        return kk.labelled(b"entropy:%d" % (len(seen) - 1), nbytes)
    ctx.set_randombytes(rb)
    try:
        pks, sks = ctx.kem_keypair(n=n)
    finally:
        ctx.set_randombytes(None)
    assert seen == [64] * n
    for b in range(n):
        want = kk.model(k, kk.labelled(b"entropy:%d" % b, 64))
        _same(k, n, b, "pk", pks[b], want[0])
        _same(k, n, b, "sk", sks[b], want[1])
    a, b_ = ctx.kem_keypair(n=n), ctx.kem_keypair(n=n)
    assert len(set(a[0]) | set(b_[0])) == 2 * n and len(set(s[-32:] for s in a[1] + b_[1])) == 2 * n
    for pks, sks in (a, b_):
        assert ctx.kem_check_sk(sks) == [0] * n and ctx.kem_check_pk(pks) == [0] * n
        assert [kk.flags_sk(k, s) for s in sks] == [0] * n and [s[384 * k:768 * k + 32] for s in sks] == pks


@pytest.mark.parametrize("k", KS)
def test_xof_block_limit(k, keys, torch_cuda, monkeypatch):
    """a handle whose gen_matrix may squeeze three SHAKE128 blocks per entry: a batch that holds a four-block item anywhere returns
    the "block limit" error and leaves device outputs untouched; the very next call without such an item gives the model's keys"""
    from mpcith_kyber_kosk_amd import api
    torch = torch_cuda
    v = keys[k]
    four = v["fx"]["four_block"]
    plain = [i for i in range(kk.ITEMS) if i not in four]
    monkeypatch.setenv("KOSK_DEBUG_XOF_BLOCKS", "3")
    ctx = api.Kosk(kyber_k=k, max_batch=1)
    monkeypatch.delenv("KOSK_DEBUG_XOF_BLOCKS")
    try:
        for n, pos in ((1, 0), (70, 0), (70, 37), (70, 69)):
            idx = plain[:n]
            idx[pos] = four[0]
            coins = [v["coins"][i] for i in idx]
            with pytest.raises(api.KoskError, match="block limit"):
                ctx.kem_keypair(coins)
            d_pk = torch.full((n * ctx.pk_bytes,), SENTINEL, dtype=torch.uint8, device="cuda")
            d_sk = torch.full((n * ctx.sk_bytes,), SENTINEL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            with pytest.raises(api.KoskError, match="block limit"):
                ctx.kem_keypair(coins, out=(d_pk.data_ptr(), d_sk.data_ptr()))
            torch.cuda.synchronize()
            assert bool((d_pk == SENTINEL).all()) and bool((d_sk == SENTINEL).all()), (k, n, pos)
            good = plain[:n]
            pks, sks = ctx.kem_keypair([v["coins"][i] for i in good])  # the error word was cleared
            assert pks == [v["pk"][i] for i in good] and sks == [v["sk"][i] for i in good], (k, n)
    finally:
        ctx.close()


@pytest.mark.parametrize("k", KS)
def test_flow_keypair_enc_dec_and_proofs(k, handles, keys, torch_cuda):
    """kem_keypair, kem_enc, kem_dec give equal secrets; key pairs made into device buffers and handed on as device pointers to
    prove_keys are all proven, and the proofs verify under the public keys"""
    torch = torch_cuda
    ctx, v = handles[k], keys[k]
    n = 5
    pks, sks = ctx.kem_keypair(v["coins"][:n])
    cts, sss = ctx.kem_enc(pks, [kk.labelled(b"flow:m:%d" % i, 32) for i in range(n)])
    assert ctx.kem_dec(cts, sks) == sss and len(set(sss)) == n
    m = 3
    d_pk = torch.zeros((m * ctx.pk_bytes,), dtype=torch.uint8, device="cuda")
    d_sk = torch.zeros((m * ctx.sk_bytes,), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.kem_keypair(v["coins"][10:10 + m], out=(d_pk.data_ptr(), d_sk.data_ptr()))
    pis, ok = ctx.prove_keys(d_sk.data_ptr(), seeds=[kk.labelled(b"flow:seed:%d" % i, 32) for i in range(m)], n=m)
    assert ok == [True] * m
    pk = bytes(d_pk.cpu().numpy())
    got = [pk[b * ctx.pk_bytes:(b + 1) * ctx.pk_bytes] for b in range(m)]
    assert got == v["pk"][10:10 + m]
    assert ctx.verify(pis, got) == [True] * m


def test_resident_state_is_left_alone(keys):
    """after a verify call of 46 proofs, kem_enc_verified gives the same ciphertexts and secrets for fixed coins before and after a
    kem_keypair call (and key checks) on the handle: pk_epoch and the resident keys are not touched"""
    from mpcith_kyber_kosk_amd import api
    k, n = 2, 46
    ctx = api.Kosk(kyber_k=k, max_batch=n)
    try:
        pks, sks, pis = ctx.verifiable_keygen(seeds=[kk.labelled(b"resident:seed:%d" % i, 32) for i in range(n)])
        coins = [kk.labelled(b"resident:coins:%d" % i, 32) for i in range(n)]
        assert ctx.verify(pis, pks) == [True] * n
        first = ctx.kem_enc_verified(n, coins)
        assert first[2] == [True] * n
        kp, ks = ctx.kem_keypair(keys[k]["coins"][:100])
        assert kp == keys[k]["pk"][:100] and ks == keys[k]["sk"][:100]
        assert ctx.kem_check_sk(ks) == [0] * 100 and ctx.kem_check_pk(kp) == [0] * 100
        assert ctx.kem_enc_verified(n, coins) == first
        assert ctx.kem_dec(first[0], sks) == first[1]
    finally:
        ctx.close()


def test_argument_errors(handles, keys, torch_cuda):
    from mpcith_kyber_kosk_amd import api
    torch = torch_cuda
    k = 2
    ctx, v = handles[k], keys[k]
    d = torch.full((ctx.sk_bytes,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = ctx.path_count(api.Kosk.PATH_KEM_KEYPAIR), ctx.path_count(api.Kosk.PATH_KEM_CHECK)
    with pytest.raises(api.KoskError):
        ctx.kem_keypair(n=0)
    with pytest.raises(api.KoskError):
        ctx.kem_keypair([])
    with pytest.raises(api.KoskError):
        ctx.kem_keypair(v["coins"][:1], out=(0, d.data_ptr()))
    with pytest.raises(api.KoskError):
        ctx.kem_keypair(v["coins"][:1], out=(d.data_ptr(), 0))
    with pytest.raises(api.KoskError, match="64 bytes"):
        ctx.kem_keypair([v["coins"][0][:63]])
    with pytest.raises(api.KoskError):
        ctx.kem_check_pk([])
    with pytest.raises(api.KoskError):
        ctx.kem_check_sk([v["pk"][0]])
    torch.cuda.synchronize()
    assert bool((d == SENTINEL).all())
    assert (ctx.path_count(api.Kosk.PATH_KEM_KEYPAIR), ctx.path_count(api.Kosk.PATH_KEM_CHECK)) == before  # nothing was started
    assert ctx.kem_keypair(v["coins"][:2]) == (v["pk"][:2], v["sk"][:2])
    assert ctx.kem_check_sk(v["sk"][:2]) == [0, 0]


# ---------------------------------------------------------------------------------------------------------- key checks --
def _rehash(k, sk):
    """sk with its stored H(pk) recomputed over the pk inside it: a range flag is then the sole reason"""
    import hashlib
    pvb = 384 * k
    return sk[:2 * pvb + 32] + hashlib.sha3_256(sk[pvb:2 * pvb + 32]).digest() + sk[-32:]


@pytest.mark.parametrize("k", KS)
def test_every_field_is_looked_at(k, handles, keys):
    """item i holds q in 12-bit field i and is otherwise an honest key, for every i: in a pk (check_pk), in the pk inside an sk and in
    s-hat (check_sk).  Each lane of k_kem_check owns groups of eight fields and the wave ORs into one word: a group nobody reads, or a
    lane whose verdict does not arrive, passes a key here"""
    ctx, v = handles[k], keys[k]
    pvb, nf = 384 * k, 256 * k
    pk, sk = v["pk"][5], v["sk"][5]
    recs = [kk.set_field(pk, 0, i, Q) for i in range(nf)]
    want = [kk.flags_pk(k, r) for r in recs]
    assert want == [kk.PK_RANGE] * nf
    assert ctx.kem_check_pk(recs) == want
    recs = [kk.set_field(sk, pvb, i, Q) for i in range(nf)]
    want = [kk.flags_sk(k, r) for r in recs]
    assert want == [kk.PK_RANGE | kk.HASH] * nf
    assert ctx.kem_check_sk(recs) == want
    assert ctx.kem_check_sk([_rehash(k, r) for r in recs]) == [kk.PK_RANGE] * nf
    recs = [kk.set_field(sk, 0, i, Q) for i in range(nf)]
    want = [kk.flags_sk(k, r) for r in recs]
    assert want == [kk.S_RANGE] * nf
    assert ctx.kem_check_sk(recs) == want


@pytest.mark.parametrize("k", KS)
def test_every_byte_is_looked_at(k, handles, keys):
    """one flipped bit per byte of the pk inside the sk (n = pk_bytes > KEM_WAVE_MAX for K = 3, 4: the per-lane H(pk); the first 512
    again as a call of their own: the wave sponge), per byte of the stored H(pk) and per byte of z (which no check reads).  The
    model gives the flags, including where the flipped bit also makes a field >= q"""
    ctx, v = handles[k], keys[k]
    pvb = 384 * k
    sk = v["sk"][6]
    recs = [kk.flip(sk, pvb + at) for at in range(ctx.pk_bytes)]
    want = [kk.flags_sk(k, r) for r in recs]
    assert all(w & kk.HASH for w in want) and kk.HASH | kk.PK_RANGE in want and kk.HASH in want
    assert ctx.kem_check_sk(recs) == want
    assert ctx.kem_check_sk(recs[:512]) == want[:512]
    recs = [kk.flip(sk, 2 * pvb + 32 + at) for at in range(32)]
    assert [kk.flags_sk(k, r) for r in recs] == [kk.HASH] * 32
    assert ctx.kem_check_sk(recs) == [kk.HASH] * 32
    recs = [kk.flip(sk, 2 * pvb + 64 + at) for at in range(32)]
    assert ctx.kem_check_sk(recs) == [0] * 32
    # s-hat bytes too: S_RANGE exactly where the flipped bit makes a field >= q
    recs = [kk.flip(sk, at) for at in range(pvb)]
    want = [kk.flags_sk(k, r) for r in recs]
    assert set(want) == {0, kk.S_RANGE}
    assert ctx.kem_check_sk(recs) == want


@pytest.mark.parametrize("k", KS)
def test_values_at_the_edges_of_the_polynomials(k, handles, keys):
    """q - 1 passes, q and 0xFFF fail, at the first and last coefficient of every polynomial and their neighbours (both positions of a
    3-byte pair), each flag as the sole reason -- inside batches of 130 honest keys at positions 0, 63, 64 and 129, then alone"""
    ctx, v = handles[k], keys[k]
    pvb = 384 * k
    pk, sk = v["pk"][7], v["sk"][7]
    at = [256 * p + f for p in range(k) for f in (0, 1, 254, 255)]
    pk_cases = [(kk.set_field(pk, 0, f, val), 0 if val < Q else kk.PK_RANGE) for f in at for val in (Q - 1, Q, 0xFFF)]
    sk_cases = [(kk.set_field(sk, 0, f, val), 0 if val < Q else kk.S_RANGE) for f in at for val in (Q - 1, Q, 0xFFF)]
    sk_cases += [(_rehash(k, kk.set_field(sk, pvb, f, val)), 0 if val < Q else kk.PK_RANGE) for f in at for val in (Q - 1, Q, 0xFFF)]
    sk_cases += [(kk.flip(sk, 2 * pvb + 32 + b), kk.HASH) for b in (0, 31)]
    sk_cases += [(kk.set_field(sk, pvb, f, Q - 1), kk.HASH) for f in (0, 256 * k - 1)]  # an in-range change of the pk: the hash alone
    for rec, want in pk_cases:
        assert kk.flags_pk(k, rec) == want
    for rec, want in sk_cases:
        assert kk.flags_sk(k, rec) == want
    for cases, fn, honest in ((pk_cases, ctx.kem_check_pk, v["pk"]), (sk_cases, ctx.kem_check_sk, v["sk"])):
        for first in range(0, len(cases), len(POSITIONS)):
            part = cases[first:first + len(POSITIONS)]
            recs, want = list(honest), [0] * kk.ITEMS
            for pos, (rec, w) in zip(POSITIONS, part):
                recs[pos], want[pos] = rec, w
            assert fn(recs) == want, (k, first)
        for i, (rec, w) in enumerate(cases):
            assert fn([rec]) == [w], (k, i)


@pytest.mark.parametrize("k", KS)
def test_enc_still_folds_a_flagged_key(k, handles):
    """the enc edges of tests/golden/kem_edges_v1.json whose t-hat is all q or all 0xFFF are flagged by kem_check_pk, and kem_enc
    still returns what that fixture pins for them: the checks are separate calls, enc keeps folding"""
    ctx = handles[k]
    fx = ke.load()["k"]["k%d" % k]["enc"]
    edges = ke.enc_edges(k)
    assert [e[0] for e in edges] == ["that_fff", "that_zero", "that_qm1", "that_q"]
    assert ctx.kem_check_pk([e[1] for e in edges]) == [kk.PK_RANGE, 0, 0, kk.PK_RANGE]
    cts, sss = ctx.kem_enc([e[1] for e in edges], [e[2] for e in edges])
    for ct, ss, rec in zip(cts, sss, fx):
        assert kf.sha3(ct) == rec["ct"] and ss.hex() == rec["ss"]


def test_check_counter_counts_launch_groups(handles, keys):
    from mpcith_kyber_kosk_amd import api
    k = 2
    ctx, v = handles[k], keys[k]
    c0 = ctx.path_count(api.Kosk.PATH_KEM_CHECK)
    kp0 = ctx.path_count(api.Kosk.PATH_KEM_KEYPAIR)
    assert ctx.kem_check_pk(v["pk"][:3]) == [0] * 3
    assert ctx.path_count(api.Kosk.PATH_KEM_CHECK) == c0 + 1
    n = CHUNK + 3
    recs = [v["sk"][b % kk.ITEMS] for b in range(n)]
    recs[CHUNK - 1] = kk.set_field(recs[CHUNK - 1], 0, 3, Q)
    recs[CHUNK] = kk.flip(recs[CHUNK], len(recs[CHUNK]) - 40)
    recs[n - 1] = kk.set_field(recs[n - 1], 384 * k, 0, 0xFFF)
    want = [0] * n
    want[CHUNK - 1], want[CHUNK], want[n - 1] = kk.S_RANGE, kk.HASH, kk.HASH | kk.PK_RANGE
    assert [kk.flags_sk(k, recs[b]) for b in (CHUNK - 1, CHUNK, n - 1)] == [want[b] for b in (CHUNK - 1, CHUNK, n - 1)]
    assert ctx.kem_check_sk(recs) == want
    assert ctx.path_count(api.Kosk.PATH_KEM_CHECK) == c0 + 3
    assert ctx.path_count(api.Kosk.PATH_KEM_KEYPAIR) == kp0
    assert "kem_keypair" not in ctx.path_counts() and list(ctx.path_counts()) == api.Kosk.PATH_IDS
