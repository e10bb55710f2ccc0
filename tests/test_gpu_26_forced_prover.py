"""GPU: the PROVER at forced opened lists (kosk_force_opened_candidates) -- Fiat-Shamir round 2 (k_fs_chain<FS_OPENED>, the host's
opened_from_candidates / opened_derived_tables) and the wire image (k_assemble_groups / asm_group_block) at what a list out of the hash
never is: windows with 64, 63, 46 of 46 and no opened parties, runs of 20 windows without one, probing chains of 149 steps, 149
entries that wrap from party 1453 to party 0 (tests/opened_sets.py: CATALOGUE, CANDIDATES; their shapes are pinned in
tests/test_forced_prover_host.py).

Nothing here compares GPU output with GPU output: the expected tables are the Python model's, the expected digests hashlib's, the
expected proofs the oracle's forcing prover's (ko_force_opened), byte for byte."""
import ctypes as C
import hashlib

import numpy as np
import pytest

from tests import forced_proofs as fp
from tests import opened_sets as osets

pytestmark = pytest.mark.gpu

NPARTY, NOPEN, NREST, SEL = osets.NPARTY, osets.NOPEN, osets.NREST, 1312
FILL = 0xA5A5
CASES = list(osets.CATALOGUE) + list(osets.CANDIDATES)             # 13
FEW_K = list(fp.FEW) + ["all_1453"]                                # K = 2 and K = 4
FORMATS = ("first150", "last150", "all_1453")


@pytest.fixture(scope="module")
def torch():
    t = pytest.importorskip("torch")
    if not t.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return t


def _expected_rows(I):
    sel, rest = [FILL] * SEL, [FILL] * SEL
    for i, v in osets.sel_row(I).items():
        sel[i] = v
    rest[:NREST] = osets.tables(I)[0]
    return sel, rest


def _check_rows(what, b, sel, rest, I):
    esel, erest = _expected_rows(I)
    for row, got, exp in (("sel", list(sel), esel), ("rest", list(rest), erest)):
        if got != exp:
            at = next(i for i in range(SEL) if got[i] != exp[i])
            pytest.fail("%s: table %d: %s row differs at entry %d: %d, expected %d" % (what, b, row, at, got[at], exp[at]))


@pytest.mark.parametrize("bound", [False, True])
def test_tables_kernel_level(bound, torch):
    """k_fs_chain<FS_OPENED[, BOUND], FORCED> through kosk_fs_opened[_bound]_device on 16 random digest tables, the 13 cases forced:
    rows b < 13 are the model's tables of probe(case), whole rows; rows b >= 13 the host function's; d_ch stays the hash of the table;
    with the hook cleared every row is the honest one"""
    from mpcith_kyber_kosk_amd import api
    n_forced, n = len(CASES), len(CASES) + 3
    assert n_forced == 13
    rng = np.random.default_rng(2600 + bound)
    tables = rng.integers(0, 256, size=(n, NPARTY * 32), dtype=np.uint8)
    binds = rng.integers(0, 256, size=(n, 32), dtype=np.uint8)
    honest = []
    for b in range(n):
        I, R = (C.c_uint16 * NOPEN)(), (C.c_uint16 * NREST)()
        if bound:
            assert api.lib.kosk_fs_opened_bound(tables[b].tobytes(), binds[b].tobytes(), I, R) == 0
        else:
            assert api.lib.kosk_fs_opened(tables[b].tobytes(), I, R) == 0
        assert list(R) == osets.complement(list(I))
        honest.append(list(I))
    ctx = api.Kosk(kyber_k=3, max_batch=2)
    try:
        d_t = torch.from_numpy(tables).cuda()
        d_b = torch.from_numpy(binds).cuda()

        def run():
            d_sel = torch.full((n + 1, SEL), FILL - 65536, dtype=torch.int16, device="cuda")  # one guard row behind the last table
            d_rest = torch.full((n + 1, SEL), FILL - 65536, dtype=torch.int16, device="cuda")
            d_ch = torch.zeros((n + 1, 32), dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            if bound:
                ctx.fs_opened_bound_device(d_t.data_ptr(), NPARTY * 32, n, d_b.data_ptr(), d_sel.data_ptr(), d_rest.data_ptr(), SEL, d_ch.data_ptr())
            else:
                ctx.fs_opened_device(d_t.data_ptr(), NPARTY * 32, n, d_sel.data_ptr(), d_rest.data_ptr(), SEL, d_ch.data_ptr())
            ctx.synchronize()
            sel, rest, ch = d_sel.cpu().numpy().view(np.uint16), d_rest.cpu().numpy().view(np.uint16), d_ch.cpu().numpy()
            assert (sel[n] == FILL).all() and (rest[n] == FILL).all() and not ch[n].any()
            for b in range(n):
                msg = tables[b].tobytes() + (binds[b].tobytes() if bound else b"")
                assert ch[b].tobytes() == hashlib.sha3_256(msg).digest(), b
            return sel, rest

        ctx.force_opened_candidates([fp.candidates(name) for name in CASES])
        sel, rest = run()
        for b, name in enumerate(CASES):
            _check_rows("forced " + name, b, sel[b], rest[b], osets.probe(fp.candidates(name)))
        for b in range(n_forced, n):
            _check_rows("behind the lists", b, sel[b], rest[b], honest[b])
        ctx.force_opened_candidates(None)
        sel, rest = run()
        for b in range(n):
            _check_rows("cleared", b, sel[b], rest[b], honest[b])
    finally:
        ctx.close()


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


def _check_proofs(oracle, k, names, got, what):
    pks, sks, pis = got
    p = oracle.params(k)
    for b, name in enumerate(names):
        opk, osk, opi = fp.forced(k, name)
        assert pks[b] == opk and sks[b] == osk, (what, name)
        if pis[b] != opi:
            pytest.fail("%s: proof %d, forced list %s: %s; opened per window %r" % (
                what, b, name, _where(p, pis[b], opi), osets.windows(osets.probe(fp.candidates(name)))))


@pytest.mark.parametrize("fs", [0, 1])
@pytest.mark.parametrize("k", [2, 3, 4])
def test_forced_proofs_equal_the_oracles(k, fs, oracle, torch):
    """verifiable_keygen under forcing: pk, sk and the proof image of every case equal the oracle's forcing prover's; with the hook
    cleared the same handle returns the oracle's honest proof"""
    from mpcith_kyber_kosk_amd import api
    names = CASES if k == 3 else FEW_K
    ctx = api.Kosk(kyber_k=k, max_batch=len(names), fs_mode=fs)
    try:
        ctx.force_opened_candidates([fp.candidates(name) for name in names])
        got = ctx.verifiable_keygen([fp.tape(k, name) for name in names])
        _check_proofs(oracle, k, names, got, "k=%d fs=%d" % (k, fs))
        ctx.force_opened_candidates(None)
        pks, sks, pis = ctx.verifiable_keygen([fp.tape(k, names[0])])
        opk, osk, opi = fp.honest(k, fp.tape_index(k, names[0]))
        assert pks[0] == opk and sks[0] == osk
        assert pis[0] == opi, "k=%d fs=%d: cleared: %s" % (k, fs, _where(oracle.params(k), pis[0], opi))
    finally:
        ctx.close()


@pytest.mark.parametrize("fs", [0, 1])
def test_forced_lists_follow_the_proofs_across_chunks(fs, oracle, torch):
    """max_batch = 3 and 13 proofs: chunks of 3 and a last one of 1, list first + b for proof b of a chunk; then tapes and lists reversed"""
    from mpcith_kyber_kosk_amd import api
    k = 3
    assert len(CASES) > 3 and len(CASES) % 3
    ctx = api.Kosk(kyber_k=k, max_batch=3, fs_mode=fs)
    try:
        for names in (CASES, CASES[::-1]):
            ctx.force_opened_candidates([fp.candidates(name) for name in names])
            got = ctx.verifiable_keygen([fp.tape(k, name) for name in names])
            _check_proofs(oracle, k, names, got, "chunks of 3, fs=%d, from %s" % (fs, names[0]))
    finally:
        ctx.close()


@pytest.mark.parametrize("k", [2, 3, 4])
def test_forced_proofs_in_the_compact_and_dense_formats(k, oracle, torch):
    from mpcith_kyber_kosk_amd import api
    lib = api.lib
    cb = lib.kosk_compact_proof_bytes(k)
    ctx = api.Kosk(kyber_k=k, max_batch=len(FORMATS))
    try:
        ctx.force_opened_candidates([fp.candidates(name) for name in FORMATS])
        tapes = [fp.tape(k, name) for name in FORMATS]
        cpk, csk, blobs = ctx.verifiable_keygen_compact(tapes)
        dpk, dsk, recs = ctx.verifiable_keygen_dense(tapes)
        for b, name in enumerate(FORMATS):
            opk, osk, opi = fp.forced(k, name)
            assert cpk[b] == opk and csk[b] == osk and dpk[b] == opk and dsk[b] == osk, (k, name)
            want = C.create_string_buffer(cb)
            assert lib.kosk_proof_compress(k, opi, want) == 0
            assert blobs[b] == want.raw, "k=%d %s: compact proof differs at byte %d" % (
                k, name, next(i for i in range(cb) if blobs[b][i] != want.raw[i]))
            rc, rec = api.dense_pack(k, opi)
            assert rc == 0, (k, name, rc)
            assert recs[b] == rec, "k=%d %s: dense proof differs at byte %d" % (
                k, name, next(i for i in range(len(rec)) if recs[b][i] != rec[i]))
    finally:
        ctx.close()


def test_refusals(oracle, torch):
    from mpcith_kyber_kosk_amd import api
    k = 3
    names = list(fp.FEW)
    tapes = [fp.tape(k, name) for name in names]
    ctx = api.Kosk(kyber_k=k, max_batch=3)
    try:
        ctx.force_opened_candidates([fp.candidates(name) for name in names[:2]])
        with pytest.raises(api.KoskError, match="fewer forced candidate lists"):
            ctx.verifiable_keygen(tapes)                                   # three proofs, two lists
        bad = list(fp.candidates(names[2]))
        bad[149] = NPARTY
        with pytest.raises(api.KoskError, match="not a party"):
            ctx.force_opened_candidates([fp.candidates(names[0]), bad])
        for n in (0, -1, 4097):
            with pytest.raises(api.KoskError, match="KOSK_FORCE_MAX_LISTS"):
                ctx.force_opened_candidates([fp.candidates(names[0])], n=n)
        # the refused calls changed nothing: two lists are still set
        _check_proofs(oracle, k, names[:2], ctx.verifiable_keygen(tapes[:2]), "after the refusals")
    finally:
        ctx.close()
    member = api.Kosk(kyber_k=k, max_batch=2, combine=2)
    try:
        with pytest.raises(api.KoskError, match="cohort member"):
            member.force_opened_candidates([fp.candidates(names[0])])
        pks, sks, pis = member.verifiable_keygen(tapes[:1])               # and it proves as it always did
        assert (pks[0], sks[0], pis[0]) == fp.honest(k, fp.tape_index(k, names[0]))
    finally:
        member.close()
