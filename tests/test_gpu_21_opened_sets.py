"""GPU: the verifier at FORCED opened lists -- every edge of its set-up and interpolation kernels (k_opened_setup, k_disassemble_fields,
k_interp_setup, k_gather_frags, k_interp_apply) that a list out of the Fiat-Shamir hash never reaches: no holes, 150 holes, hi at its
maximum, lo = 150 (every point but the last in the below-lo branch), runs of hole points, empty 64-party windows (tests/opened_sets.py).

The oracle's forcing prover (ko_force_opened) opens a chosen list; such a proof is consistent in every check except the last one,
I' == I, which the oracle makes last ("Check failed for reom_I...") and the GPU verifier reports as fail bit 11 on its own.  So the oracle
reaches its last check exactly when the GPU's fail mask is 1 << 11 and nothing else: any other bit on an intact forced proof is an error
of the set-up or the interpolation at that list, and the bit names the check."""
import ctypes as C
import time

import pytest

from tests import opened_sets as osets

pytestmark = pytest.mark.gpu

FB_MALFORMED, FB_OPENED_SET = 0, 11
ONLY_OPENED_SET = 1 << FB_OPENED_SET
REOM = "Check failed for reom_I"
FEW = ("first150", "run100_249", "mid600_749")  # the sets that also run at K = 2 and K = 4 (K = 4: 52 and 32 interpolated columns)


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return torch


def _oracle_verify_many(oracle, cases):
    """the oracle's (verdict, reason) on many (k, pi, pk), a few at a time, as in test_gpu_02_verify.py (ctypes releases the interpreter
    lock; the oracle's verifier has no shared mutable state once its tables exist -- the caller has verified one proof before)"""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(6) as ex:
        return list(ex.map(lambda c: oracle.kosk_verify(*c), cases))


@pytest.fixture(scope="module")
def forced(oracle):
    """{k: {"honest": (pk, pi), "sets": {name: (pk, pi)}}}: the forced proofs, made once by the oracle (its hook is process-wide, so
    one after the other) and never changed; the oracle's verdict on every forced proof is taken here."""
    from tests import forced_proofs  # the same proofs serve the forcing prover's tests: made once per process
    t0 = time.time()
    out = {}
    for k in (2, 3, 4):
        names = list(osets.CATALOGUE) if k == 3 else list(FEW)
        hpk, _, hpi = forced_proofs.honest(k)
        sets = {}
        for name in names:
            pk, _, pi = forced_proofs.forced(k, name)
            sets[name] = (pk, pi)
        out[k] = {"honest": (hpk, hpi), "sets": sets}
    out["prove_seconds"] = time.time() - t0
    for k in (2, 3, 4):
        assert oracle.kosk_verify(k, *out[k]["honest"][::-1])[0]  # (the tables are built here, by one thread)
    cases = [(k, name) for k in (2, 3, 4) for name in out[k]["sets"]]
    verdicts = _oracle_verify_many(oracle, [(k, out[k]["sets"][name][1], out[k]["sets"][name][0]) for k, name in cases])
    for (k, name), (ok, why) in zip(cases, verdicts):
        assert not ok and why.startswith(REOM), (k, name, why)  # every other check of the oracle's verifier holds
    out["oracle_seconds"] = time.time() - t0
    print("forced proofs: %.1f s proving, %.1f s with the oracle's verdicts" % (out["prove_seconds"], out["oracle_seconds"]))
    return out


def _batch(forced, k):
    """every forced proof of this K with the honest one in front, in the middle and at the end -> (labels, pks, pis)"""
    f = forced[k]
    items = [(name,) + f["sets"][name] for name in f["sets"]]
    mid = len(items) // 2
    hon = ("honest",) + f["honest"]
    items = [hon] + items[:mid] + [hon] + items[mid:] + [hon]
    return [x[0] for x in items], [x[1] for x in items], [x[2] for x in items]


def _expect(labels, got, masks, what):
    for lab, g, m in zip(labels, got, masks):
        if lab == "honest":
            assert g is True and m == 0, (what, lab, g, hex(m))
        else:
            assert g is False and m == ONLY_OPENED_SET, "%s: forced list %s: verify bit %s, fail mask %#x (expected %#x alone): %r" % (
                what, lab, g, m, ONLY_OPENED_SET, osets.shape(osets.CATALOGUE[lab]))


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("fs", [0, 1])
@pytest.mark.parametrize("k", [2, 3, 4])
def test_intact_forced_proofs(k, fs, strict, forced, torch_cuda):
    from mpcith_kyber_kosk_amd import api
    labels, pks, pis = _batch(forced, k)
    ctx = api.Kosk(kyber_k=k, max_batch=len(pis), fs_mode=fs, strict_encoding=strict)
    try:
        got = ctx.verify(pis, pks)
        _expect(labels, got, ctx.fail_masks(len(pis)), "k=%d fs=%d strict=%d" % (k, fs, strict))
    finally:
        ctx.close()


@pytest.mark.parametrize("k", [2, 3, 4])
def test_intact_forced_proofs_chunked_and_reversed(k, forced, torch_cuda):
    """kosk_verify_batch on a handle of max_batch = 3: the batch goes in chunks, the last one ragged; then the same batch reversed:
    w, l(k), node_of, hrange and the window counts are indexed per proof"""
    from mpcith_kyber_kosk_amd import api
    labels, pks, pis = _batch(forced, k)
    if len(pis) % 3 == 0:  # keep the last chunk ragged
        labels, pks, pis = labels + labels[1:2], pks + pks[1:2], pis + pis[1:2]
    assert len(pis) > 3 and len(pis) % 3
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    try:
        got = ctx.verify(pis, pks)
        _expect(labels, got, ctx.fail_masks(len(pis)), "k=%d chunks of 3" % k)
        got = ctx.verify(pis[::-1], pks[::-1])
        _expect(labels[::-1], got, ctx.fail_masks(len(pis)), "k=%d chunks of 3, reversed" % k)
    finally:
        ctx.close()
    ctx = api.Kosk(kyber_k=k, max_batch=len(pis))
    try:
        got = ctx.verify(pis[::-1], pks[::-1])
        _expect(labels[::-1], got, ctx.fail_masks(len(pis)), "k=%d reversed" % k)
    finally:
        ctx.close()


@pytest.mark.parametrize("k", [2, 3, 4])
def test_intact_forced_proofs_compact_and_dense(k, forced, torch_cuda):
    """the compact and the dense verify calls.  Every forced image is a codeword of the dense format (its dropped rows ARE the
    interpolation of the kept ones), so dense_pack takes it, and after verify_dense the resident images are the original ones byte for
    byte: the GPU refill on real codewords at these lists."""
    from mpcith_kyber_kosk_amd import api
    lib = api.lib
    labels, pks, pis = _batch(forced, k)
    n = len(pis)
    cb = lib.kosk_compact_proof_bytes(k)
    blobs = []
    for pi in pis:
        out = C.create_string_buffer(cb)
        assert lib.kosk_proof_compress(k, pi, out) == 0
        blobs.append(out.raw)
    recs = []
    for lab, pi in zip(labels, pis):
        rc, rec = api.dense_pack(k, pi)
        assert rc == 0, (k, lab, rc)
        recs.append(rec)
    ctx = api.Kosk(kyber_k=k, max_batch=n)
    try:
        ok = C.create_string_buffer(n)
        assert lib.kosk_verify_batch_compact(ctx.handle, n, b"".join(blobs), b"".join(pks), ok) == 0
        _expect(labels, [b == 1 for b in ok.raw], ctx.fail_masks(n), "k=%d compact" % k)
        got = ctx.verify_dense(recs, pks)
        _expect(labels, got, ctx.fail_masks(n), "k=%d dense" % k)
        back = ctx.fetch_proofs(n)
        for lab, a, b in zip(labels, back, pis):
            assert a == b, "k=%d %s: the resident image after unpack + refill differs from the original at byte %d" % (
                k, lab, next(i for i in range(len(b)) if a[i] != b[i]))
    finally:
        ctx.close()


# unopened-record indices per field: first node, last node of the set the field is interpolated over, first record behind the nodes, last record
TAMPER_AT = {13: (0, 406, 407, 1303),  # s + r: every record is compared
             8: (0, 406, 407),         # t
             15: (406, 407),           # s_eta
             21: (0, 812, 813)}        # u_s: degree 2d
MESSAGE_BIT = (("beta[", 1), ("s + r share error", 2), ("e + r share error", 2), ("for t[", 5), ("_eta[", 7), (".u[", 9), ("u2d[", 10))


@pytest.mark.parametrize("name", list(osets.CATALOGUE))
def test_tampers_placed_relative_to_the_set(name, forced, oracle, torch_cuda):
    """K = 3, one u16 replaced by another canonical residue at the first node, the last node, the first record behind the nodes: the
    oracle decides whether the record is read at all (its reason stays the last check: the GPU mask stays 1 << 11 alone) or which check
    breaks first (the GPU mask holds that bit beside bit 11, and never bit 0)."""
    from mpcith_kyber_kosk_amd import api
    k = 3
    p = oracle.params(k)
    pk, pi = forced[k]["sets"][name]
    rest = osets.complement(osets.CATALOGUE[name])
    width = {f: p.size[f] // 2 // 1304 for f in (2, 8, 13, 15, 21)}
    assert width == {2: 70, 8: k, 13: k, 15: k * 5, 21: k * 4}
    where = [(f, i) for f, at in TAMPER_AT.items() for i in at]
    if rest[0] < 407:
        where.append((2, 0))                                              # beta of the first unopened party below 407
    where.append((2, next(i for i, q in enumerate(rest) if q >= 407)))    # and of the first one at or above: never read
    bad = []
    for f, i in where:
        t = bytearray(pi)
        o = p.off[f] + 2 * i * width[f]
        t[o:o + 2] = ((int.from_bytes(t[o:o + 2], "little") + 1) % 3329).to_bytes(2, "little")
        bad.append(bytes(t))
    ctx = api.Kosk(kyber_k=k, max_batch=len(bad) + 1)
    try:
        got = ctx.verify(bad + [pi], [pk] * (len(bad) + 1))
        masks = ctx.fail_masks(len(bad) + 1)
    finally:
        ctx.close()
    exp = _oracle_verify_many(oracle, [(k, t, pk) for t in bad])
    assert got == [False] * (len(bad) + 1) and masks[-1] == ONLY_OPENED_SET, (got, [hex(m) for m in masks])
    unread = read = 0
    for (f, i), m, (e, why) in zip(where, masks, exp):
        what = "%s: field %d record %d: mask %#x, oracle: %s" % (name, f, i, m, why)
        print(what)
        assert not e, what
        if why.startswith(REOM):
            unread += 1
            assert m == ONLY_OPENED_SET, what
            continue
        read += 1
        assert m & ONLY_OPENED_SET and m & ~ONLY_OPENED_SET and not m & (1 << FB_MALFORMED), what
        for text, bit in MESSAGE_BIT:
            if text in why:
                assert m & (1 << bit), what
    assert unread >= 3 and read >= 9, (unread, read)  # the sample holds both kinds
