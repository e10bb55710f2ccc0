"""The verifier's DEFAULT mode (kosk_options::strict_encoding = 1) at every field and edge: a u16 >= q in a record the reference reads
sets fail bit 0, records the reference never reads stay unchecked.

Every expectation comes from tests/strict_model.py -- the read set restated from the reference's line numbers and pinned to the oracle
by tests/test_strict_model.py -- and from the oracle, never from the library.  One default and one strict_encoding = 0 handle per K,
max_batch = 64; every verify call is a chunk of at most 64 proofs, so that fail_masks belongs to the chunk."""
import pytest

from tests import strict_model as sm

pytestmark = pytest.mark.gpu

Q = sm.Q
CHUNK = 64


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return torch


@pytest.fixture(scope="module")
def handles(torch_cuda):
    """{k: (default handle, reference-following handle)}, created at first use"""
    from mpcith_kyber_kosk_amd import api
    made = {}

    def get(k):
        if k not in made:
            made[k] = (api.Kosk(kyber_k=k, max_batch=CHUNK), api.Kosk(kyber_k=k, max_batch=CHUNK, strict_encoding=0))
        return made[k]
    yield get
    for pair in made.values():
        for h in pair:
            h.close()


def _verify_chunks(ctx, images, pk):
    """verify bits and fail masks of many proofs under one key, chunk by chunk; `images` yields the proofs"""
    bits, masks, chunk = [], [], []

    def flush():
        bits.extend(ctx.verify(chunk, [pk] * len(chunk)))
        masks.extend(ctx.fail_masks(len(chunk)))
        del chunk[:]
    for img in images:
        chunk.append(img)
        if len(chunk) == CHUNK:
            flush()
    if chunk:
        flush()
    return bits, masks


def _bump(m, pi, f, rec, elem):
    """the same residue, non-canonical: v + q in place of v (v < q: fits 16 bits)"""
    idx = m.index(f, rec, elem)
    v = m.get(pi, f, idx)
    assert v < Q
    return m.put(pi, f, idx, v + Q)


def _sweep_cases(m):
    """{(field, record, element): (window, first record of the window, what)} of the edge sweep.  Unopened fields: the aligned 64-party
    ranges w = 0 .. 22, window w = records #{rest < 64 w} .. #{rest < 64 (w + 1)} - 1; opened fields: records 0-63, 64-127, 128-149."""
    cases = {}
    start = [sum(1 for q in m.rest if q < 64 * w) for w in range(24)]
    assert start[0] == 0 and start[23] == sm.NREST
    for f in sm.U16_FIELDS:
        w_ = m.width[f]
        wins = [(0, 64), (64, 128), (128, sm.NOPEN)] if f in sm.OPENED_FIELDS else [(start[w], start[w + 1]) for w in range(23)]
        for w, (i0, i1) in enumerate(wins):
            if i1 <= i0:
                continue
            cases.setdefault((f, i0, 0), (w, i0, "start"))
            cases.setdefault((f, i1 - 1, w_ - 1), (w, i0, "end"))
        if f in sm.LIMITED_FIELDS:  # either side of the limit, first and last element of both records
            for rec, what in zip(m.limit_records(f), ("last read", "first unread")):
                w, i0 = next((w, a) for w, (a, b) in enumerate(wins) if a <= rec < b)
                cases.setdefault((f, rec, 0), (w, i0, what))
                cases.setdefault((f, rec, w_ - 1), (w, i0, "end" if what == "last read" else what))
    for f in (0, 6):  # the widest field (most dwords per lane) and the narrowest: the middle of a chunk
        cases.setdefault((f, 96, m.width[f] // 2), (1, 64, "middle"))
    return cases


def _riffle(a, b):
    """a and b merged so that both kinds are spread evenly over the whole list"""
    keyed = [((i + 0.25) / len(a), x) for i, x in enumerate(a)] + [((j + 0.75) / len(b), x) for j, x in enumerate(b)]
    return [x for _, x in sorted(keyed, key=lambda t: t[0])]


@pytest.mark.parametrize("k", [2, 3, 4])
def test_strict_range_check_at_every_window_edge(k, oracle, handles):
    """Honest GPU proof of tape 133 + k; exactly + q (the same residue: the reference's ZZ_p / gf3329_mul uses cannot tell) on the first
    element of the first record and the last element of the last record of every 64-party window of every unopened u16 field and of
    every 64-record chunk of every opened one, on the first and last element of the records on either side of each limit, and in the
    middle of a chunk of fields 0 and 6.  Default handle: bit 0 with mask & 1 where the model says read, bit 1 with mask 0 where it
    says unread.  Read and unread cases alternate inside every chunk of 64, whose positions 0 and 63 hold the untouched proof: the
    flag is per proof, not per launch.

    The elements at a window's start sit at an odd u16 offset from a 4-byte boundary -- (off[f] + 2 i0 width) % 4 == 2 -- only where
    a record has an odd number of u16 and i0 is odd; every field offset is a multiple of 4 and the opened chunks start at even records,
    so that needs an unopened field of odd width: K = 3 (widths 3 and 15).  For K = 2 and K = 4 every width of an unopened field is
    even and no window of any proof can start or end off a 4-byte boundary; the test asserts both alignments for K = 3, and for every K
    that each alignment the layout can produce was bumped."""
    p = oracle.params(k)
    strict, _ = handles(k)
    pks, _, pis = strict.verifiable_keygen([oracle.tape_bytes_for(k, sm.TAPE + k)])
    pk, pi = pks[0], pis[0]
    m = sm.ReadSet(p, *sm.opened_list(p, pi))
    assert m.strict_expectation(pi) == {}
    cases = _sweep_cases(m)
    read = [c for c in cases if m.read(c[0], c[1])]
    unread = [c for c in cases if not m.read(c[0], c[1])]
    # what the test asserts about its own inputs
    assert {c[0] for c in read} == set(sm.U16_FIELDS) and len(sm.U16_FIELDS) == 21
    assert {c[0] for c in unread} == set(sm.LIMITED_FIELDS) and len(sm.LIMITED_FIELDS) == 7
    odd_start = lambda f, i0: (p.off[f] + 2 * i0 * m.width[f]) % 4 == 2
    head = {odd_start(c[0], cases[c][1]) for c in read if cases[c][2] == "start"}  # a window's very first element
    possible = {odd_start(c[0], cases[c][1]) for c in cases}
    assert head == possible and False in head, (head, possible)
    # the last element of a window (or of its part up to the last read record) lies behind the window's last whole dword exactly when
    # the u16 from its first whole dword on are odd in number
    tail = {((c[1] + 1 - cases[c][1]) * m.width[c[0]] - odd_start(c[0], cases[c][1])) % 2 == 1 for c in read if cases[c][2] == "end"}
    if k == 3:
        assert head == {False, True} and tail == {False, True}
    else:
        assert tail == {False}
        assert all(p.off[f] % 4 == 0 for f in sm.U16_FIELDS) and all(m.width[f] % 2 == 0 for f in sm.UNOPENED_FIELDS)
    order = _riffle(read, unread)
    per = CHUNK - 2
    chunks = [order[i:i + per] for i in range(0, len(order), per)]
    assert all(any(m.read(c[0], c[1]) for c in ch) and any(not m.read(c[0], c[1]) for c in ch) for ch in chunks)

    def images():
        for ch in chunks:
            yield pi
            for c in ch:
                yield _bump(m, pi, *c)
            for _ in range(CHUNK - 1 - len(ch)):  # the last chunk is filled up with the untouched proof: position 63 of every chunk
                yield pi
    bits, masks = _verify_chunks(strict, images(), pk)
    assert len(bits) == CHUNK * len(chunks)
    wrong = []
    for n, ch in enumerate(chunks):
        row = [None] + list(ch) + [None] * (CHUNK - 1 - len(ch))
        for pos, c in enumerate(row):
            bit, mask = bits[n * CHUNK + pos], masks[n * CHUNK + pos]
            if c is None:
                if not (bit and mask == 0):
                    wrong.append((k, "untouched proof", "chunk %d position %d" % (n, pos), bit, hex(mask)))
                continue
            rd = m.read(c[0], c[1])
            if (rd and not (not bit and mask & 1)) or (not rd and not (bit and mask == 0)):
                wrong.append((k, c[0], cases[c][0], c[1], c[2], "read" if rd else "unread", bit, hex(mask)))
    assert not wrong, "%d of %d: (K, field, window, record, element, read?, got bit, mask)\n%s" % (
        len(wrong), len(order), "\n".join(map(str, wrong)))


@pytest.mark.parametrize("k", [2, 3, 4])
def test_canonical_residues_at_the_read_set_edges_match_the_oracle_in_both_modes(k, oracle, handles):
    """The boundary set of tests/test_strict_model.py (same proof, same positions, verdicts from the same function): another CANONICAL
    residue at the first and last record of every field and on both sides of every limit.  Nothing here is >= q, so the default and
    the reference-following handle must both give the oracle's bit, with mask 0 exactly for the accepted: the values of a window's
    first, last and last-read records, not only their range flag."""
    pk, pi, m, cases, want = sm.boundary_set(oracle, k)
    assert m.strict_expectation(pi) == {} and 0 < sum(want) < len(want)
    for name, ctx in zip(("default", "strict_encoding=0"), handles(k)):
        bits, masks = _verify_chunks(ctx, (sm.residue_image(m, pi, *c) for c in cases), pk)
        wrong = [(k, name, f, rec, elem, "read" if m.read(f, rec) else "unread", bit, hex(mask), exp)
                 for (f, rec, elem), bit, mask, exp in zip(cases, bits, masks, want) if bit != exp or (mask == 0) != bit]
        assert not wrong, "(K, handle, field, record, element, read?, got bit, mask, oracle bit)\n%s" % "\n".join(map(str, wrong))


# (tape, items) for oracle_lib.crafted_verifiable_keygen, from CRAFTS and the list of
# tests/test_gpu_02_verify.py::test_verify_crafted_hash_consistent_non_canonical_proofs: per K two the reference accepts and one it rejects
S_1200 = (305, ((0, 0, 1200, 1),))                                   # one raw s share of an opened party
F0_15Q = (311, tuple((2, 0, q, 15) for q in range(3, 1454, 11)))     # f_0 + 15 q: raw beta, gamma chains >= q
NTTF71 = (312, tuple((3, 71, q, 3) for q in range(0, 1454, 7)))      # NTT f_71, the base of NTT_r
F0_NTTF71 = (315, tuple((2, 0, q, 9) for q in range(1, 1454, 9)) + tuple((3, 71, q, 12) for q in range(1, 1454, 9)))
S_RAW = (316, tuple((0, 0, q, 1) for q in range(0, 1454, 7)))        # raw s shares everywhere: s + r shares >= q among the unopened
E_11 = (300, ((1, 1, 11, 2),))                                       # rejected at NTT(e)
STRICT_CRAFTS = {2: (S_1200, F0_15Q, S_RAW), 3: (F0_15Q, NTTF71, E_11), 4: (F0_15Q, F0_NTTF71, S_RAW)}
UNOPENED_CRAFT = ((2, 0, 1400, 15),)  # on a tape whose proof leaves party 1400 unopened no element >= q reaches the image


@pytest.mark.parametrize("k", [2, 3, 4])
def test_default_rejects_crafted_hash_consistent_proofs_the_reference_accepts(k, oracle, handles):
    """The malleability attack itself: proofs by the oracle's crafting prover, every hash consistent with the u16 >= q they hold.  The
    reference (oracle) ACCEPTS at least two of them per K; the default handle rejects every one with a read element >= q (bit 0,
    mask & 1), the reference-following handle gives the oracle's bit.  A craft whose party stays unopened leaves a canonical image:
    both handles accept it."""
    p = oracle.params(k)
    strict, lax = handles(k)
    crafts = []
    for tidx, items in STRICT_CRAFTS[k]:
        pk, _, pi = oracle.crafted_verifiable_keygen(k, oracle.tape_bytes_for(k, tidx), list(items))
        crafts.append((tidx, pk, pi))
    expect = [sm.ReadSet(p, *sm.opened_list(p, pi)).strict_expectation(pi) for _, _, pi in crafts]
    want = [oracle.kosk_verify(k, pi, pk)[0] for _, pk, pi in crafts]
    assert all(expect), expect
    assert sum(want) >= 2 and not all(want), "fewer than two crafts the reference accepts with a read u16 >= q: %s" % (want,)
    for tidx in (320, 321, 322):
        pk, _, pi = oracle.crafted_verifiable_keygen(k, oracle.tape_bytes_for(k, tidx), list(UNOPENED_CRAFT))
        if not sm.ReadSet(p, *sm.opened_list(p, pi)).strict_expectation(pi):
            assert oracle.kosk_verify(k, pi, pk)[0]
            crafts.append((tidx, pk, pi)); expect.append({}); want.append(True)
            break
    pis, pks = [c[2] for c in crafts], [c[1] for c in crafts]
    got_s, mask_s = strict.verify(pis, pks), strict.fail_masks(len(pis))
    got_l, mask_l = lax.verify(pis, pks), lax.fail_masks(len(pis))
    for (tidx, _, _), e, w, gs, ms, gl, ml in zip(crafts, expect, want, got_s, mask_s, got_l, mask_l):
        what = "K=%d tape %d, read u16 >= q per field %s, oracle %s" % (k, tidx, e, w)
        assert gl == w and (ml == 0) == gl, "%s: strict_encoding=0 handle bit %s mask %#x" % (what, gl, ml)
        if e:
            assert not gs and ms & 1, "%s: default handle bit %s mask %#x" % (what, gs, ms)
        else:
            assert gs and ms == 0, "%s: default handle bit %s mask %#x" % (what, gs, ms)


WAYS_K, WAYS_TAPE = 3, 146  # the last s + r record of this proof holds an element below 767 (asserted)


def ways_in_cases(oracle, pk, pi):
    """[read-record bump, unread bump, honest] and the same for the compact wire (12-bit values: a bump that stays below 4096)"""
    p = oracle.params(WAYS_K)
    m = sm.ReadSet(p, *sm.opened_list(p, pi))
    assert m.read(13, sm.NREST - 1) and not m.read(8, 407)
    unread = _bump(m, pi, 8, 407, 0)
    plain = [_bump(m, pi, 13, sm.NREST - 1, m.width[13] - 1), unread, pi]
    small = [e for e in range(m.width[13]) if m.get(pi, 13, m.index(13, sm.NREST - 1, e)) < 4096 - Q]
    assert small, "no element below 767 in the last record of field 13"
    # kosk_proof_compress refuses the image whichever record holds the value >= 4096: the first small element behind record 406 of field 8
    rec, elem = next((r, e) for r in range(407, sm.NREST) for e in range(m.width[8]) if m.get(pi, 8, m.index(8, r, e)) < 4096 - Q)
    wire = [_bump(m, pi, 13, sm.NREST - 1, small[0]), _bump(m, pi, 8, rec, elem), pi]
    for imgs in (plain, wire):
        assert [bool(m.strict_expectation(t)) for t in imgs] == [True, False, False]
    return plain, wire


def _inst(api, k, seed64):
    """the mlwe_inst image (A, t, s, e) of kyber_keygen on seed64"""
    _, _, A, s, e, t = api.host_keygen(k, seed64)
    return A.tobytes() + t.tobytes() + s.tobytes() + e.tobytes()


def test_strict_default_on_every_way_in(oracle, torch_cuda):
    """K = 3: a + q in a read record (field 13, last record, last element), one in an unread record (field 8, record 407) and the
    honest proof give [False, True, True] with masks[0] & 1 through every entry point that leads to the verifier, and
    kosk_kem_enc_verified encapsulates only where the bit is 1."""
    import ctypes as C
    from mpcith_kyber_kosk_amd import api
    from tests import kem_fixture as kf
    k = WAYS_K
    tape = oracle.tape_bytes_for(k, WAYS_TAPE)
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    pks, _, pis = ctx.verifiable_keygen([tape])
    pks = pks * 3
    plain, wire = ways_in_cases(oracle, pks[0], pis[0])
    want = [False, True, True]
    for t in plain + wire:  # the same residues: the reference accepts all of them outside the s + r comparison of the first
        assert oracle.kosk_verify(k, t, pks[0])[0] == (t not in (plain[0], wire[0])), oracle.kosk_verify(k, t, pks[0])

    def check(what, bits, h=ctx):
        masks = h.fail_masks(3)
        assert bits == want and masks[0] & 1 and masks[1:] == [0, 0], (what, bits, [hex(x) for x in masks])
    check("verify", ctx.verify(plain, pks))
    coins = [bytes([i]) * 32 for i in range(3)]
    cts, sss, done = ctx.kem_enc_verified(3, coins)
    ref_ct, ref_ss = ctx.kem_enc(pks, coins)
    assert done == want and cts[0] == bytes(kf.CT_BYTES[k]) and sss[0] == bytes(32)
    assert (cts[1:], sss[1:]) == (ref_ct[1:], ref_ss[1:])
    ctx.stage_verifier_inputs(plain, pks)
    check("stage_verifier_inputs + verify_resident", ctx.verify_resident(3))
    ctx.stage_verifier_inputs([pis[0]] * 3, pks)
    assert ctx.verify_resident_pk(3, pks=pks) == [True] * 3
    ctx.stage_verifier_inputs(plain, pks)
    check("verify_resident_pk", ctx.verify_resident_pk(3, pks=pks))
    check("verify_inst", ctx.verify_inst(plain, [_inst(api, k, tape[:64])] * 3))
    # the compact wire
    cb = api.lib.kosk_compact_proof_bytes(k)
    blobs = []
    for t in wire:
        out = C.create_string_buffer(cb)
        assert api.lib.kosk_proof_compress(k, t, out) == 0
        blobs.append(out.raw)
    ok = C.create_string_buffer(3)
    assert api.lib.kosk_verify_batch_compact(ctx.handle, 3, b"".join(blobs), b"".join(pks), ok) == 0
    check("verify_batch_compact", [b == 1 for b in ok.raw])
    ctx.stage_verifier_inputs_compact(blobs, pks)
    check("stage_verifier_inputs_compact + verify_resident", ctx.verify_resident(3))
    ctx.close()
    dev = api.Kosk(kyber_k=k, max_batch=3, fs_mode=api.FS_DEVICE)
    check("fs_mode=FS_DEVICE verify", dev.verify(plain, pks), dev)
    dev.stage_verifier_inputs(plain, pks)
    check("fs_mode=FS_DEVICE verify_resident", dev.verify_resident(3), dev)
    assert dev.path_counts()["fs_device"] > 0 and dev.path_counts()["fs_host"] == 0
    dev.close()
    lax = api.Kosk(kyber_k=k, max_batch=3, strict_encoding=0)  # the reference-following mode rejects the first for the reference's reason
    assert lax.verify(plain, pks) == want and lax.fail_masks(3)[0] & 1 == 0
    lax.close()


def test_strict_default_in_merged_runs(torch_cuda, gpu_child):
    out = gpu_child("from tests.gpu_child_strict import merged_runs_keep_their_mode; merged_runs_keep_their_mode()")
    assert "merged_runs_keep_their_mode ok" in out
