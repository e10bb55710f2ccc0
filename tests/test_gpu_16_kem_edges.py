"""GPU tests of the Kyber KEM calls at their edges, against tests/golden/kem_edges_v1.json and kem_vectors_v1.json (what the
reference's crypto_kem_enc_derand / crypto_kem_dec returned) and hashlib for rejection keys.  Every comparison is exact and covers every
item of every batch.  tests/test_kem_edges_host.py checks the same fixture against the device functions built for the host: where that
passes and a test here fails, the fault is in how the kernels deal out the work or in the host code, not in kosk_kem_dev.hpp.

  a  edge vectors    12-bit fields >= q in pk and sk, ciphertexts that enc never made, what dec takes from the sk, rare ends of the
                     rejection sampling -- inside batches of ordinary items and alone
  b  every ct byte   one flipped bit per byte position, next to the untouched ciphertext
  c  sizes           KEM_WAVE_MAX - 1, KEM_WAVE_MAX, KEM_WAVE_MAX + 1, 17 waves - 1
  d  growth          the workspace allocated, grown (freed and allocated again), then used below its capacity
  e  device buffers  across a launch group
  f  block limit     gen_matrix's error return in both calls, and that it does not stick
  g  verified mask   kosk_kem_enc_verified over more than one wave of proofs
(h, the per-lane sponge roles at K = 2 and 4, is in tests/test_gpu_14_kem.py::test_per_lane_sponges_on_small_batches.)"""
import hashlib

import pytest

from tests import kem_edges as ke
from tests import kem_fixture as kf

pytestmark = pytest.mark.gpu

KS = (2, 3, 4)
CHUNK = 16384        # KEM_CHUNK of csrc/kosk_ctx.hpp: items per launch group
WAVE_MAX = 1024      # KEM_WAVE_MAX: up to here H(pk) and rkprf run one wave per item, above it one lane per item inside k_kem_hash
SENTINEL = 0xA5
N_MIXED = 130        # three waves of items in every role of k_kem_hash, edge items in each of them
ENC_POS = (0, 31, 63, 64, 65, 100, 127, 129)                        # 4 enc edges + 4 sampling keys; 0 and n - 1 included
DEC_POS = tuple(sorted((0, 63, 64, 65, 127, 128, 129) + tuple(range(3, 123, 7))))  # 21 dec edges + 4 sampling keys


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


def _first_diff(got, want):
    return next((j for j in range(len(want)) if got[j] != want[j]), None)


def _same(k, n, b, name, what, got, want):
    """got == want (bytes), or a failure that names K, batch size, position, item and the first differing byte"""
    if got != want:
        at = _first_diff(got, want)
        pytest.fail("K=%d n=%d position %d (%s): first differing %s byte %d: %02x, expected %02x" % (k, n, b, name, what, at, got[at], want[at]))


def _same_ct(k, n, b, name, got, item):
    if "ct_hex" in item:
        _same(k, n, b, name, "ct", got, bytes.fromhex(item["ct_hex"]))
    assert kf.sha3(got) == item["ct"], "K=%d n=%d position %d (%s): ct digest differs" % (k, n, b, name)


class Inputs:
    """per K, computed once and never modified: the ordinary items (kem_vectors_v1.json) with their regenerated keys, and the edge
    items of kem_edges_v1.json as (name, inputs ..., expected) lists.  The ciphertexts that dec needs as inputs are not in the
    fixtures: they come from kem_enc on the GPU and are checked against the recorded digests before use."""

    def __init__(self, k, ctx):
        self.k = k
        self.items = kf.load()["k"]["k%d" % k]
        keys = [kf.keypair(k, i) for i in range(kf.ITEMS)]
        for i, it in enumerate(self.items):
            assert kf.sha3(keys[i][0]) == it["pk"] and kf.sha3(keys[i][1]) == it["sk"]
        self.pk = [kf.enc_pk(k, i) for i in range(kf.ITEMS)]
        self.sk = [s for _, s in keys]
        self.m = [kf.message(k, i) for i in range(kf.ITEMS)]
        self.dec_want = [bytes.fromhex(it["dec_ss"] if i == 2 else it["ss"]) for i, it in enumerate(self.items)]
        fx = ke.load()["k"]["k%d" % k]
        self.fx = fx
        # enc edges: (name, pk, m, fixture record)
        self.enc = [(name, pk, m, rec) for (name, pk, m), rec in zip(ke.enc_edges(k), fx["enc"])]
        self.sampling = []
        for (cond, idx, m), rec in zip(ke.sampling_edges(k), fx["sampling"]):
            assert rec["cond"] == cond and rec["index"] == idx
            pk, sk = kf.keypair(k, idx)
            self.sampling.append(("sampling_" + cond, pk, m, rec, sk))
        self.enc += [s[:4] for s in self.sampling]
        # the ciphertexts dec needs: of every ordinary item, of the honest key, of the sampling keys
        cts, sss = ctx.kem_enc(self.pk, self.m)
        for i, it in enumerate(self.items):
            _same_ct(k, kf.ITEMS, i, "item %d" % i, cts[i], it)
        self.ct = cts
        (ct_valid,), (ss_valid,) = ctx.kem_enc([ke.valid_input(k)[0]], [ke.valid_input(k)[1]])
        assert kf.sha3(ct_valid) == fx["valid"]["ct"] and ss_valid.hex() == fx["valid"]["ss"], "K=%d: the valid ciphertext of the dec edges" % k
        # dec edges: (name, ct, sk, expected ss)
        self.dec = [(name, ct, sk, bytes.fromhex(rec["ss"])) for (name, ct, sk), rec in zip(ke.dec_edges(k, ct_valid), fx["dec"])]
        assert [d[0] for d in self.dec] == [rec["name"] for rec in fx["dec"]]
        s_cts, s_sss = ctx.kem_enc([s[1] for s in self.sampling], [s[2] for s in self.sampling])
        for s, ct, ss in zip(self.sampling, s_cts, s_sss):
            assert kf.sha3(ct) == s[3]["ct"] and ss.hex() == s[3]["ss"], "K=%d %s" % (k, s[0])
            self.dec.append((s[0], ct, s[4], ss))
        assert len(self.enc) == len(ENC_POS) and len(self.dec) == len(DEC_POS) == len(set(DEC_POS))


@pytest.fixture(scope="module")
def inputs(handles):
    return {k: Inputs(k, handles[k]) for k in KS}


def _check_by_position(k, v, cts, sss, n):
    for b in range(n):
        _same_ct(k, n, b, "item %d" % (b % kf.ITEMS), cts[b], v.items[b % kf.ITEMS])
        assert sss[b].hex() == v.items[b % kf.ITEMS]["ss"], (k, n, b)


def _enc_dec_by_position(ctx, k, v, n):
    """enc then dec of n items, item b % ITEMS at position b (items 0-3 included), every position against the fixture"""
    idx = [b % kf.ITEMS for b in range(n)]
    cts, sss = ctx.kem_enc([v.pk[i] for i in idx], [v.m[i] for i in idx])
    _check_by_position(k, v, cts, sss, n)
    got = ctx.kem_dec(cts, [v.sk[i] for i in idx])
    for b, i in enumerate(idx):
        _same(k, n, b, "item %d" % i, "dec ss", got[b], v.dec_want[i])


# ---------------------------------------------------------------------------------------------------------------- a --
@pytest.mark.parametrize("k", KS)
def test_edge_vectors_in_a_batch_and_alone(k, handles, inputs):
    """all enc edges in one kem_enc call and all dec edges in one kem_dec call, among ordinary items (n = 130: every role of
    k_kem_hash spans three waves, and edge items sit in each, at block 0 and at block n - 1); then each edge item alone"""
    ctx, v = handles[k], inputs[k]
    n = N_MIXED
    # enc
    pks, ms, names, want = list(v.pk), list(v.m), ["item %d" % i for i in range(n)], list(v.items)
    for pos, (name, pk, m, rec) in zip(ENC_POS, v.enc):
        pks[pos], ms[pos], names[pos], want[pos] = pk, m, name, rec
    cts, sss = ctx.kem_enc(pks, ms)
    for b in range(n):
        _same_ct(k, n, b, names[b], cts[b], want[b])
        _same(k, n, b, names[b], "ss", sss[b], bytes.fromhex(want[b]["ss"]))
    for name, pk, m, rec in v.enc:
        (ct,), (ss,) = ctx.kem_enc([pk], [m])
        _same_ct(k, 1, 0, name, ct, rec)
        _same(k, 1, 0, name, "ss", ss, bytes.fromhex(rec["ss"]))
    # dec
    dcts, sks, names, want = list(v.ct), list(v.sk), ["item %d" % i for i in range(n)], list(v.dec_want)
    for pos, (name, ct, sk, ss) in zip(DEC_POS, v.dec):
        dcts[pos], sks[pos], names[pos], want[pos] = ct, sk, name, ss
    got = ctx.kem_dec(dcts, sks)
    for b in range(n):
        _same(k, n, b, names[b], "dec ss", got[b], want[b])
    for name, ct, sk, ss in v.dec:
        _same(k, 1, 0, name, "dec ss", ctx.kem_dec([ct], [sk])[0], ss)
    # what the edge items are worth: the accept is an accept, every other result is the rejection key of the z stored in that sk
    accepts = [name for name, ct, sk, ss in v.dec if ss != hashlib.shake_256(sk[-32:] + ct).digest(32)]
    assert accepts == ["shat_plus_q"] + ["sampling_" + c for c in ke.CONDS]


# ---------------------------------------------------------------------------------------------------------------- b --
@pytest.mark.parametrize("k", KS)
def test_every_ciphertext_byte_is_compared(k, handles, inputs):
    """item 3's ciphertext with bit at % 8 of byte at flipped, for every at, at the odd positions of one kem_dec call; the untouched
    ciphertext at the even ones.  Each of the (K + 1) 32 work items of encrypt_block owns a byte range of the comparison and all 256
    threads OR into one LDS word: a range that is not compared, or a wave whose difference does not arrive, accepts a tampered
    ciphertext here.  n = 2 CT_BYTES > KEM_WAVE_MAX, so the rkprf runs per lane; the first 512 positions again as a call of their
    own put tampered ciphertexts through k_kem_rkprf_wave."""
    ctx, v = handles[k], inputs[k]
    it = v.items[ke.TAMPER_ITEM]
    ct3, sk3, ss3 = bytes.fromhex(it["ct_hex"]), v.sk[ke.TAMPER_ITEM], bytes.fromhex(it["ss"])
    cts, want = [], []
    for t in ke.tamper_all(ct3):
        cts += [ct3, t]
        want += [ss3, hashlib.shake_256(sk3[-32:] + t).digest(32)]
    n = len(cts)
    assert n == 2 * kf.CT_BYTES[k] > WAVE_MAX
    h = hashlib.sha3_256()
    for w in want[1::2]:
        h.update(w)
    assert h.hexdigest() == v.fx["tamper_all"]["digest"]  # what the reference returned for these ciphertexts
    for m in (n, 512):
        got = ctx.kem_dec(cts[:m], [sk3] * m)
        for b in range(m):
            _same(k, m, b, "untouched" if b % 2 == 0 else "byte %d tampered" % (b // 2), "dec ss", got[b], want[b])


# ---------------------------------------------------------------------------------------------------------------- c --
@pytest.mark.parametrize("n", (WAVE_MAX - 1, WAVE_MAX, WAVE_MAX + 1, 17 * 64 - 1))
@pytest.mark.parametrize("k", KS)
def test_sizes_around_the_wave_sponge_limit(k, n, handles, inputs):
    """in process, without KOSK_DEBUG_KEM_WAVE_MAX: the last two sizes of the wave-sponge layout and the first of the per-lane one.
    Above the limit n is no multiple of 64, so waves of k_kem_hash straddle two roles (rkprf | gen_matrix, H(pk) + G | gen_matrix)."""
    _enc_dec_by_position(handles[k], k, inputs[k], n)


# ---------------------------------------------------------------------------------------------------------------- d --
@pytest.mark.parametrize("k", KS)
def test_workspace_growth(k, torch_cuda, inputs, oracle):
    """a fresh handle whose first KEM call already needs 2048 items of workspace, then 2049 (freed and allocated again at 3072), then
    calls far below and just inside the capacity; afterwards the proving pipeline on the handle still equals the oracle"""
    from mpcith_kyber_kosk_amd import api
    ctx = api.Kosk(kyber_k=k, max_batch=1)
    try:
        for n in (WAVE_MAX + 1, 2 * WAVE_MAX + 1, 3, WAVE_MAX + 1):
            _enc_dec_by_position(ctx, k, inputs[k], n)
        tape = oracle.tape_bytes_for(k, 2)
        pks, sks, pis = ctx.verifiable_keygen([tape])
        opk, osk, opi, _, _ = oracle.verifiable_keygen(k, tape)
        assert (pks[0], sks[0], pis[0]) == (opk, osk, opi)
        assert ctx.verify(pis, pks) == [True]
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------- e --
def test_device_buffers_across_a_launch_group(handles, inputs, torch_cuda):
    """K = 2, n = KEM_CHUNK + 3: every input and output a device buffer, so the second launch group works at `pointer + first * size`
    of device memory; a sentinel margin around every output"""
    torch = torch_cuda
    k, n, pad = 2, CHUNK + 3, 64
    ctx, v = handles[k], inputs[k]
    ctb = kf.CT_BYTES[k]
    idx = [b % kf.ITEMS for b in range(n)]
    dev = lambda blobs: torch.frombuffer(bytearray(b"".join(blobs)), dtype=torch.uint8).cuda()
    d_pk, d_sk, d_m = dev([v.pk[i] for i in idx]), dev([v.sk[i] for i in idx]), dev([v.m[i] for i in idx])
    d_ct = torch.full((pad + n * ctb + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_ss = torch.full((pad + n * 32 + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    d_ss2 = torch.full((pad + n * 32 + pad,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.kem_enc(d_pk.data_ptr(), d_m.data_ptr(), n=n, out=(d_ct.data_ptr() + pad, d_ss.data_ptr() + pad))
    ctx.kem_dec(d_ct.data_ptr() + pad, d_sk.data_ptr(), n=n, out=d_ss2.data_ptr() + pad)
    ct, ss, ss2 = bytes(d_ct.cpu().numpy()), bytes(d_ss.cpu().numpy()), bytes(d_ss2.cpu().numpy())
    for buf in (ct, ss, ss2):
        assert buf[:pad] == bytes([SENTINEL]) * pad and buf[-pad:] == bytes([SENTINEL]) * pad
    cts = [ct[pad + b * ctb:pad + (b + 1) * ctb] for b in range(n)]
    sss = [ss[pad + b * 32:pad + (b + 1) * 32] for b in range(n)]
    _check_by_position(k, v, cts, sss, n)
    for b, i in enumerate(idx):
        _same(k, n, b, "item %d" % i, "dec ss", ss2[pad + b * 32:pad + (b + 1) * 32], v.dec_want[i])
    # the last item of the first launch group and the first and last of the second: the same bytes as a host-buffer call of the three
    at = [CHUNK - 1, CHUNK, CHUNK + 2]
    h_ct, h_ss = ctx.kem_enc([v.pk[idx[b]] for b in at], [v.m[idx[b]] for b in at])
    assert h_ct == [cts[b] for b in at] and h_ss == [sss[b] for b in at]
    assert ctx.kem_dec(h_ct, [v.sk[idx[b]] for b in at]) == [ss2[pad + b * 32:pad + (b + 1) * 32] for b in at]


# ---------------------------------------------------------------------------------------------------------------- f --
@pytest.mark.parametrize("k", KS)
def test_xof_block_limit_in_the_kem_calls(k, handles, inputs, torch_cuda, monkeypatch):
    """a handle whose gen_matrix may squeeze three SHAKE128 blocks per entry: key (d) -- every entry of A^T needs exactly three --
    gives the fixture's results in both calls; with key (a) -- one entry needs a fourth -- anywhere in the batch both calls return
    the "block limit" error and leave a device output buffer untouched; the error does not stick to the handle.  The default handle
    (32 blocks) gives the fixture's results for the keys (a), (b) and (c) (also part of test_edge_vectors_in_a_batch_and_alone)."""
    from mpcith_kyber_kosk_amd import api
    torch = torch_cuda
    v = inputs[k]
    by = {s[0][-1]: s for s in v.sampling}                          # cond -> (name, pk, m, record, sk)
    ct_of = {d[0][-1]: d[1] for d in v.dec if d[0].startswith("sampling_")}  # cond -> its ciphertext (made on the default handle)
    assert by["d"][3]["blocks"] == [3] * (k * k) and 4 in by["a"][3]["blocks"]
    monkeypatch.setenv("KOSK_DEBUG_XOF_BLOCKS", "3")
    ctx = api.Kosk(kyber_k=k, max_batch=1)
    monkeypatch.delenv("KOSK_DEBUG_XOF_BLOCKS")
    ctb = kf.CT_BYTES[k]
    _, pk_d, m_d, rec_d, sk_d = by["d"]
    _, pk_a, m_a, rec_a, sk_a = by["a"]

    def good(n):
        cts, sss = ctx.kem_enc([pk_d] * n, [m_d] * n)
        for b in range(n):
            assert kf.sha3(cts[b]) == rec_d["ct"] and sss[b].hex() == rec_d["ss"], (k, n, b)
        assert ctx.kem_dec(cts, [sk_d] * n) == sss
    try:
        good(5)
        for n, pos in ((1, 0), (70, 0), (70, 37), (70, 69)):
            pks, ms, sks, cts = [pk_d] * n, [m_d] * n, [sk_d] * n, [ct_of["d"]] * n
            pks[pos], ms[pos], sks[pos], cts[pos] = pk_a, m_a, sk_a, ct_of["a"]
            with pytest.raises(api.KoskError, match="block limit"):
                ctx.kem_enc(pks, ms)
            with pytest.raises(api.KoskError, match="block limit"):
                ctx.kem_dec(cts, sks)
            d_ct = torch.full((n * ctb,), SENTINEL, dtype=torch.uint8, device="cuda")
            d_ss = torch.full((n * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
            d_ss2 = torch.full((n * 32,), SENTINEL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            with pytest.raises(api.KoskError, match="block limit"):
                ctx.kem_enc(pks, ms, out=(d_ct.data_ptr(), d_ss.data_ptr()))
            with pytest.raises(api.KoskError, match="block limit"):
                ctx.kem_dec(cts, sks, out=d_ss2.data_ptr())
            torch.cuda.synchronize()
            for buf in (d_ct, d_ss, d_ss2):
                assert bool((buf == SENTINEL).all()), (k, n, pos)
            good(2)  # the very next calls on the same handle: the error word was cleared
    finally:
        ctx.close()
    dflt = handles[k]
    for c in ("a", "b", "c"):
        name, pk, m, rec, sk = by[c]
        (ct,), (ss,) = dflt.kem_enc([pk], [m])
        assert kf.sha3(ct) == rec["ct"] and ss.hex() == rec["ss"], (k, c)
        assert dflt.kem_dec([ct], [sk]) == [ss], (k, c)


# ---------------------------------------------------------------------------------------------------------------- g --
def test_enc_verified_mask_over_more_than_one_wave(torch_cuda):
    """kosk_kem_enc_verified after a verify call of 130 proofs of which 0, 63, 64 and 129 are damaged: `done` is False at exactly
    those, ct and ss are zero there and what kem_enc returns for the same keys and coins everywhere else"""
    from mpcith_kyber_kosk_amd import api
    k, n, damaged = 2, 130, (0, 63, 64, 129)
    ctx = api.Kosk(kyber_k=k, max_batch=n)
    try:
        pks, sks, pis = ctx.verifiable_keygen(seeds=[ke.rnd(b"verified-mask:seed:%d" % i, 32) for i in range(n)])
        coins = [ke.rnd(b"verified-mask:coins:%d" % i, 32) for i in range(n)]
        for b in damaged:
            bad = bytearray(pis[b]); bad[1000] ^= 1
            pis[b] = bytes(bad)
        ctx.stage_verifier_inputs(pis, pks)
        assert ctx.verify_resident(n) == [b not in damaged for b in range(n)]
        cts, sss, done = ctx.kem_enc_verified(n, coins)
        assert done == [b not in damaged for b in range(n)]
        want_ct, want_ss = ctx.kem_enc(pks, coins)
        for b in range(n):
            if b in damaged:
                assert cts[b] == bytes(kf.CT_BYTES[k]) and sss[b] == bytes(32), b
            else:
                _same(k, n, b, "proven key %d" % b, "ct", cts[b], want_ct[b])
                _same(k, n, b, "proven key %d" % b, "ss", sss[b], want_ss[b])
        keep = [b for b in range(n) if b not in damaged]
        assert ctx.kem_dec([cts[b] for b in keep], [sks[b] for b in keep]) == [sss[b] for b in keep]
    finally:
        ctx.close()
