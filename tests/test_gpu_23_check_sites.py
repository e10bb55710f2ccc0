"""GPU: the verifier's fail masks on proofs in which ONE site of ONE check is the only thing wrong (tests/check_sites.py) -- fail bits
1-10 of `kosk_verify_fail_masks`, set by k_check_opened, k_check_batch, the compare mode of k_ntt256 and fed by the interpolation kernels.

Every case leaves the Fiat-Shamir hashes alone (bit 11 stays clear), so the relation checks alone decide, and each case sits at an edge of
the loops and clamps that pick the sites: polynomial 0 and K - 1 (the last MAXK slot at K = 4), gate 0 and E - 1 (the last MAXE slot at
K = 2), the s and the e side, opened positions 0 / 64 / 149, secrets 0 / 63 / 64 / 255, beta / gamma columns 0 and 69, the role split of
the s + r comparison.  The expected mask is the oracle's: ko_kosk_verify_sites goes on after a failed comparison and counts the failing
sites per bit (tests/test_check_sites_host.py proves on the CPU that each case breaks its intended checks only).  The GPU's mask must
equal it exactly, on every case, path and mode: a comparison that skips one coefficient, one gate, one side or the last opened party
turns a one-site case into an accepted forgery."""
import ctypes as C
import time

import pytest

from tests import check_sites as cs

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return torch


@pytest.fixture(scope="module")
def batches(oracle, torch_cuda):
    """{k: (labels, pks, pis, masks)}: every case of this K with the honest proof in front, in the middle and at the end, and the
    oracle-derived mask of each.  The GPU proves the catalogue's tape itself: its proof is the oracle's byte for byte."""
    from mpcith_kyber_kosk_amd import api
    out, t_oracle = {}, 0.0
    for k in (2, 3, 4):
        t0 = time.time()
        b = cs.build(oracle, k)
        names = list(b["cases"])
        exp = cs.expected(oracle, k, [(b["cases"][n][1], b["cases"][n][0]) for n in names])
        t_oracle += time.time() - t0
        ctx = api.Kosk(kyber_k=k, max_batch=1)
        try:
            pks, _, pis = ctx.verifiable_keygen([oracle.tape_bytes_for(k, cs.TAPE_INDEX)])
        finally:
            ctx.close()
        assert (pks[0], pis[0]) == b["honest"], "k=%d: the GPU's proof of the catalogue's tape differs from the oracle's" % k
        items = [(n,) + b["cases"][n] + (m,) for n, (m, _) in zip(names, exp)]
        for n, _, _, m in items:
            assert m == cs.intended_mask(n), (k, n, hex(m))
        mid, hon = len(items) // 2, ("honest",) + b["honest"] + (0,)
        items = [hon] + items[:mid] + [hon] + items[mid:] + [hon]
        assert len(items) <= 100
        out[k] = tuple([x[c] for x in items] for c in range(4))
    print("check-site cases: %d + %d + %d proofs, %.1f s in the oracle" % (len(out[2][0]), len(out[3][0]), len(out[4][0]), t_oracle))
    return out


def _expect(labels, got, masks, want, what):
    bad = ["%s: verify bit %s, fail mask %#x, oracle %#x" % (lab, g, m, w)
           for lab, g, m, w in zip(labels, got, masks, want) if g is not (w == 0) or m != w]
    assert not bad and len(got) == len(masks) == len(want), "%s: %d of %d differ\n%s" % (what, len(bad), len(want), "\n".join(bad))


@pytest.mark.parametrize("k", [2, 4])
def test_one_site_cases_default_handle(k, batches, torch_cuda):
    from mpcith_kyber_kosk_amd import api
    labels, pks, pis, want = batches[k]
    ctx = api.Kosk(kyber_k=k, max_batch=len(pis))
    try:
        got = ctx.verify(pis, pks)
        _expect(labels, got, ctx.fail_masks(len(pis)), want, "k=%d" % k)
    finally:
        ctx.close()


@pytest.mark.parametrize("strict", [0, 1])
@pytest.mark.parametrize("fs", [0, 1])
def test_one_site_cases_every_mode(fs, strict, batches, torch_cuda):
    from mpcith_kyber_kosk_amd import api
    labels, pks, pis, want = batches[3]
    ctx = api.Kosk(kyber_k=3, max_batch=len(pis), fs_mode=fs, strict_encoding=strict)
    try:
        got = ctx.verify(pis, pks)
        _expect(labels, got, ctx.fail_masks(len(pis)), want, "k=3 fs=%d strict=%d" % (fs, strict))
    finally:
        ctx.close()


def test_one_site_cases_chunked_and_reversed(batches, torch_cuda):
    """a handle of max_batch = 3: the batch goes in chunks, the last one ragged; then reversed: fail[] and the public keys are per proof"""
    from mpcith_kyber_kosk_amd import api
    labels, pks, pis, want = batches[3]
    if len(pis) % 3 == 0:  # keep the last chunk ragged
        labels, pks, pis, want = labels + labels[1:2], pks + pks[1:2], pis + pis[1:2], want + want[1:2]
    assert len(pis) > 3 and len(pis) % 3
    ctx = api.Kosk(kyber_k=3, max_batch=3)
    try:
        got = ctx.verify(pis, pks)
        _expect(labels, got, ctx.fail_masks(len(pis)), want, "k=3 chunks of 3")
        got = ctx.verify(pis[::-1], pks[::-1])
        _expect(labels[::-1], got, ctx.fail_masks(len(pis)), want[::-1], "k=3 chunks of 3, reversed")
    finally:
        ctx.close()


def test_one_site_cases_compact(batches, torch_cuda):
    """kosk_verify_batch_compact on the host-compressed images (every tampered value is a canonical residue: the codec takes it)"""
    from mpcith_kyber_kosk_amd import api
    lib = api.lib
    k = 3
    labels, pks, pis, want = batches[k]
    n, cb = len(pis), lib.kosk_compact_proof_bytes(k)
    blobs = []
    for pi in pis:
        out = C.create_string_buffer(cb)
        assert lib.kosk_proof_compress(k, pi, out) == 0
        blobs.append(out.raw)
    ctx = api.Kosk(kyber_k=k, max_batch=n)
    try:
        ok = C.create_string_buffer(n)
        assert lib.kosk_verify_batch_compact(ctx.handle, n, b"".join(blobs), b"".join(pks), ok) == 0
        _expect(labels, [b == 1 for b in ok.raw], ctx.fail_masks(n), want, "k=3 compact")
    finally:
        ctx.close()
