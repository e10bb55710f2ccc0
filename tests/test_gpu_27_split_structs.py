"""GPU: kosk_prove_prepared and kosk_verify_inst on caller-made structs (tests/split_structs.py: CATALOGUE; shapes and verdict classes are
pinned in tests/test_split_structs_host.py) -- mpcith_randomness whose f / NTT_f are zero, junk or another tape's, whole constant rows
at 0, 3328, 1664, 1665 in every limb tile of both k-steps of k_lincomb_stream, single constant rows at the k-step boundary and the r
rows' constant term, share rows on no polynomial, range sharings with chosen free points, s and e at +-3328, A and t at other int16
representatives.  A tape produces none of these.

Nothing here compares GPU output with GPU output: the expected proof is the oracle's prove() on the same three images
(oracle_lib.prove_images), byte for byte, and the expected verify bit and fail mask are the oracle's all-checks verifier's
(oracle_lib.verify_inst_sites) on the oracle's proof."""
import numpy as np
import pytest

from tests import split_structs as ss

pytestmark = pytest.mark.gpu

NPARTY, NOPEN, NREST, Q = ss.NPARTY, 150, 1304, ss.Q


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return t


def _where(p, got, want):
    """the first differing byte of a proof image as text: field id, record index inside the field, byte"""
    at = next(i for i in range(len(want)) if got[i] != want[i])
    f = next((i for i in range(24) if p.off[i] <= at < p.off[i] + p.size[i]), None)
    if f is None:
        return "byte %d (outside the fields)" % at
    rel, size = at - p.off[f], p.size[f]
    rec = "unopened record %d of 1304" % (rel // (size // NREST)) if size % NREST == 0 else \
          "opened party %d of 150" % (rel // (size // NOPEN)) if size % NOPEN == 0 else "no records"
    return "field %d, %s, byte %d of the field (%d of the image): %#x, expected %#x" % (f, rec, rel, at, got[at], want[at])


def _run(ctx, oracle, k, names, what):
    """one prove_prepared call and one verify_inst call over the cases, case b at position b of the call"""
    p = oracle.params(k)
    cases = [ss.case(k, name) for name in names]
    ss.expected_all(k)   # the oracle's side of every case, once per process
    pis = ctx.prove_prepared([c["inst"] for c in cases], [c["rand"] for c in cases], [c["range"] for c in cases], [c["tape"] for c in cases])
    bad = ["%s: proof %d, case %s: %s" % (what, b, name, _where(p, pis[b], ss.expected(k, name)[0]))
           for b, name in enumerate(names) if pis[b] != ss.expected(k, name)[0]]
    if bad:
        pytest.fail("%d of %d proofs differ from the oracle's prove() on the same structs\n%s" % (len(bad), len(names), "\n".join(bad)))
    oks = ctx.verify_inst([ss.expected(k, name)[0] for name in names], [c["inst"] for c in cases])
    masks = ctx.fail_masks(len(names))
    for b, name in enumerate(names):
        _, bit, sites = ss.expected(k, name)
        assert (oks[b], masks[b]) == (bit, ss.mask_of(sites)), "%s: verify_inst of proof %d, case %s: (%r, %#x), the oracle has (%r, %#x)" % (
            what, b, name, oks[b], masks[b], bit, ss.mask_of(sites))


@pytest.mark.parametrize("k,fs", [(3, 0), (3, 1), (2, 0), (4, 0)])
def test_catalogue_as_one_batch(k, fs, oracle, torch):
    """case b at batch position b of a handle with max_batch = len(catalogue)"""
    from mpcith_kyber_kosk_amd import api
    names = ss.names(k)
    ctx = api.Kosk(kyber_k=k, max_batch=len(names), fs_mode=fs)
    try:
        _run(ctx, oracle, k, names, "k=%d fs=%d, one batch" % (k, fs))
    finally:
        ctx.close()


@pytest.mark.parametrize("fs", [0, 1])
def test_catalogue_reversed_in_chunks_of_three(fs, oracle, torch):
    """max_batch = 3: chunks of 3, 3, ... and a last short one, the catalogue in reversed order"""
    from mpcith_kyber_kosk_amd import api
    k = 3
    names = ss.NAMES[::-1]
    assert len(names) > 3 and len(names) % 3
    ctx = api.Kosk(kyber_k=k, max_batch=3, fs_mode=fs)
    try:
        _run(ctx, oracle, k, names, "fs=%d, reversed, chunks of 3" % fs)
    finally:
        ctx.close()


def test_verify_inst_at_caller_made_instances(oracle, torch):
    """the honest proof against instances whose A and t are other int16 representatives, whose t is off by 1 or by q, whose s and e are
    junk (never read): bit and mask are the oracle's, which compares encode_to_gf3329(t) unreduced (mlwe_verifier.cpp:358)"""
    from mpcith_kyber_kosk_amd import api
    k = 3
    b = ss.base(k)
    A, t, s, e = ss.parse_inst(k, b["inst"])
    wide = lambda a, m: (a.astype(np.int32) + m * Q).astype(np.int16)
    t1, tq = t.copy(), t.copy()
    t1[1, 77] += 1
    tq[k - 1, 255] += Q
    junk = np.random.default_rng(2701).integers(-32768, 32768, size=s.shape).astype(np.int16)
    insts = {"honest": (A, t, s, e), "A - q": (wide(A, -1), t, s, e), "A + 8q": (wide(A, 8), t, s, e), "A largest": (ss.largest_int16(A), t, s, e),
             "t - q": (A, wide(t, -1), s, e), "t + 8q": (A, wide(t, 8), s, e), "t one +1": (A, t1, s, e), "t one +q": (A, tq, s, e),
             "s, e junk": (A, t, junk, junk[::-1].copy()), "t to [0, q)": (A, (t.astype(np.int32) % Q).astype(np.int16), s, e),
             "t to [-q, 0)": (A, (t.astype(np.int32) % Q - Q).astype(np.int16), s, e)}
    images = [ss.inst_image(*v) for v in insts.values()]
    want = [oracle.verify_inst_sites(k, b["pi"], img) for img in images]
    assert want[0] == (True, [0] * 12) and want[8] == (True, [0] * 12)      # the control, and s / e are not read
    assert not want[6][0] and ss.mask_of(want[6][1]) == 1 << 5              # a different residue: check 5 alone
    ctx = api.Kosk(kyber_k=k, max_batch=len(images))
    try:
        oks = ctx.verify_inst([b["pi"]] * len(images), images)
        masks = ctx.fail_masks(len(images))
        for i, name in enumerate(insts):
            assert (oks[i], masks[i]) == (want[i][0], ss.mask_of(want[i][1])), "instance %d (%s): (%r, %#x), the oracle has (%r, %#x) %r" % (
                i, name, oks[i], masks[i], want[i][0], ss.mask_of(want[i][1]), want[i][1])
    finally:
        ctx.close()


def _poke_u16(img, off, value):
    out = bytearray(img)
    out[off:off + 2] = int(value).to_bytes(2, "little")
    return bytes(out)


def test_refusals(oracle, torch):
    """rc -1 with a text for a share value >= q and for an s or e coefficient that encode_to_gf3329 leaves outside [0, q); the handle
    then proves the honest case as the oracle does"""
    from mpcith_kyber_kosk_amd import api
    k = 3
    p = oracle.params(k)
    b = ss.base(k)
    M, KE = p.M, k * p.E
    y = lambda row, party: row * ss.SHARE_VEC_BYTES + 8 + 2 * NPARTY + 2 * party   # share_y[party] of share_vec `row` of an array
    f_sh, ntt_f_sh = M * 1024, M * 1024 + M * ss.SHARE_VEC_BYTES
    places = {"f_shares[0] party 0": ("rand", f_sh + y(0, 0)), "NTT_f_shares[M-1] party 1453": ("rand", ntt_f_sh + y(M - 1, NPARTY - 1)),
              "s_eta_shares[0][0] party 0": ("range", y(0, 0)), "last e_eta_shares row party 1453": ("range", y(2 * KE - 1, NPARTY - 1))}
    ctx = api.Kosk(kyber_k=k, max_batch=2)
    try:
        def honest_still_proves(after):
            pi = ctx.prove_prepared([b["inst"]], [b["rand"]], [b["range"]], [b["tape"]])[0]
            assert pi == b["pi"], "after the refusal of %s: %s" % (after, _where(p, pi, b["pi"]))

        honest_still_proves("nothing")
        for name, (member, off) in places.items():
            for value in (3329, 0xFFFF) if member == "rand" or "last" in name else (3329,):
                imgs = dict(b)
                assert int.from_bytes(imgs[member][off:off + 2], "little") < Q
                imgs[member] = _poke_u16(imgs[member], off, value)
                with pytest.raises(api.KoskError, match="non-canonical share value"):
                    ctx.prove_prepared([b["inst"], imgs["inst"]], [b["rand"], imgs["rand"]], [b["range"], imgs["range"]], [b["tape"]] * 2)
                honest_still_proves("%s = %d" % (name, value))
        A, t, s, e = ss.parse_inst(k, b["inst"])
        for value in (3329, -3329, 32767, -32768):
            for who in (0, 1):
                s2, e2 = s.copy(), e.copy()
                if who:
                    e2[k - 1, 255] = value
                else:
                    s2[0, 0] = value
                with pytest.raises(api.KoskError, match="s or e coefficient outside"):
                    ctx.prove_prepared([ss.inst_image(A, t, s2, e2)], [b["rand"]], [b["range"]], [b["tape"]])
                honest_still_proves("%s = %d" % ("e" if who else "s", value))
        # 3328 and -3328 at the same places are field elements: proven, and as the oracle proves them
        s2, e2 = s.copy(), e.copy()
        s2[0, 0], e2[k - 1, 255] = 3328, -3328
        inst = ss.inst_image(A, t, s2, e2)
        pi = ctx.prove_prepared([inst], [b["rand"]], [b["range"]], [b["tape"]])[0]
        want = oracle.prove_images(k, inst, b["rand"], b["range"], b["tape"])
        assert pi == want, _where(p, pi, want)
    finally:
        ctx.close()
