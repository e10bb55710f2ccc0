"""GPU tests of the offline bank (kosk_bank_reserve / _level / _fill, kosk_stage_prover_keys_banked,
kosk_prove_keys_banked_batch, kosk_verifiable_keygen_banked_batch).  The reference of every comparison is the existing non-banked call
of the same handle on the spliced tape (key seed || offline section of the fill's tape || online section of the consuming call's tape),
and every comparison is exact.  One handle per test, max_batch = 4, capacity = 6; the cases with more than one handle run in a child
process (tests/gpu_child_bank.py)."""
import ctypes as C

import pytest

from tests import bank_cases as bc
from tests import keyproof_cases as kc

pytestmark = pytest.mark.gpu

KS = bc.KS


@pytest.fixture(scope="module")
def torch_cuda():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU: torch.cuda.is_available() is False")
    return torch


def _api():
    from mpcith_kyber_kosk_amd import api
    return api


def _handle(k, **opts):
    h = _api().Kosk(kyber_k=k, max_batch=bc.MAX_BATCH, **opts)
    h.bank_reserve(bc.CAPACITY)
    assert h.bank_level() == (0, bc.CAPACITY)
    return h


def _same(got, want, what):
    assert len(got) == len(want), what
    for b, (g, w) in enumerate(zip(got, want)):
        assert g == w, (what, b, bc.first_diff(g, w))


@pytest.mark.parametrize("fs", [0, 1])
@pytest.mark.parametrize("k", KS)
def test_parity_on_the_same_tape(k, fs, torch_cuda):
    """fill(tapes) then the banked call on the same tapes = kosk_prove_keys_batch on those tapes, byte for byte, in both Fiat-Shamir modes"""
    n = 3
    h = _handle(k, fs_mode=fs)
    tapes, sks = [bc.tape(k, i) for i in range(n)], bc.sks(k, n)
    want, want_ok = h.prove_keys(sks, tapes=tapes)
    h.bank_fill(tapes=tapes)
    assert h.bank_level() == (n, bc.CAPACITY)
    got, ok = h.prove_keys_banked(sks, tapes=tapes)
    assert ok == want_ok == [True] * n
    _same(got, want, ("parity", k, fs))
    assert h.verify(got, bc.pks(k, n)) == [True] * n
    assert h.bank_level() == (0, bc.CAPACITY)
    h.close()


@pytest.mark.parametrize("k", KS)
def test_splice_of_two_tapes_and_of_two_seeds(k, torch_cuda):
    api = _api()
    n = 3
    h = _handle(k)
    sks = bc.sks(k, n)
    A, B = [bc.tape(k, i, "a") for i in range(n)], [bc.tape(k, i, "b") for i in range(n)]
    want, _ = h.prove_keys(sks, tapes=[bc.splice(k, a, b) for a, b in zip(A, B)])
    pure_a, _ = h.prove_keys(sks, tapes=A)
    pure_b, _ = h.prove_keys(sks, tapes=B)
    h.bank_fill(tapes=A)
    got, ok = h.prove_keys_banked(sks, tapes=B)
    assert ok == [True] * n
    _same(got, want, ("splice of tapes", k))
    for b in range(n):
        assert got[b] != pure_a[b] and got[b] != pure_b[b]
    assert h.verify(got, bc.pks(k, n)) == [True] * n
    # seeds on both sides: "the tape" is kosk-seedtape-v1(seed)
    SA, SB = [bc.seed(k, i, "a") for i in range(n)], [bc.seed(k, i, "b") for i in range(n)]
    TA, TB = [api.tape_from_seed(k, s) for s in SA], [api.tape_from_seed(k, s) for s in SB]
    want, _ = h.prove_keys(sks, tapes=[api.tape_splice(k, a, b) for a, b in zip(TA, TB)])
    h.bank_fill(seeds=SA)
    got, ok = h.prove_keys_banked(sks, seeds=SB)
    assert ok == [True] * n
    _same(got, want, ("splice of seeds", k))
    h.close()


@pytest.mark.parametrize("k", KS)
def test_fifo_order_and_the_ring(k, torch_cuda):
    """fill 4, prove 3, fill 4 (wraps: level 5), fill 2 refused, one chunked call of 5: proof j is the reference on the splice with offline
    tape j for j = 0..7; the last slot of the allocation is used; ids 25 / 26 move by the number of chunks"""
    api = _api()
    h = _handle(k)
    put0, take0 = h.path_count(api.Kosk.PATH_BANK_PUT), h.path_count(api.Kosk.PATH_BANK_TAKE)
    off = [bc.tape(k, j, "off") for j in range(8)]
    on = [bc.tape(k, j, "on") for j in range(8)]
    sks = bc.sks(k, 8)
    want = []
    for first in (0, 4):
        w, ok = h.prove_keys(sks[first:first + 4], tapes=[bc.splice(k, off[j], on[j]) for j in range(first, first + 4)])
        assert ok == [True] * 4
        want += w
    h.bank_fill(tapes=off[0:4])                               # slots 0..3
    assert h.bank_level() == (4, bc.CAPACITY)
    got, _ = h.prove_keys_banked(sks[0:3], tapes=on[0:3])     # slots 0..2 go
    assert h.bank_level() == (1, bc.CAPACITY)
    h.bank_fill(tapes=off[4:8])                               # slots 4, 5 -- the last of the allocation -- then 0, 1
    assert h.bank_level() == (5, bc.CAPACITY)
    with pytest.raises(api.KoskError):
        h.bank_fill(tapes=off[0:2])
    assert h.bank_level() == (5, bc.CAPACITY)
    assert (h.path_count(api.Kosk.PATH_BANK_PUT) - put0, h.path_count(api.Kosk.PATH_BANK_TAKE) - take0) == (2, 1)
    more, ok = h.prove_keys_banked(sks[3:8], tapes=on[3:8])   # two chunks, 4 + 1: slots 3, 4, 5, 0 and then 1
    assert ok == [True] * 5
    _same(got + more, want, ("fifo", k))
    assert h.bank_level() == (0, bc.CAPACITY)
    assert (h.path_count(api.Kosk.PATH_BANK_PUT) - put0, h.path_count(api.Kosk.PATH_BANK_TAKE) - take0) == (2, 3)
    h.close()


@pytest.mark.parametrize("k", KS)
def test_underflow_consumes_and_writes_nothing(k, torch_cuda):
    api = _api()
    lib = api.lib
    h = _handle(k)
    off, on, sks = [bc.tape(k, j, "off") for j in range(2)], [bc.tape(k, j, "on") for j in range(3)], bc.sks(k, 3)
    want, _ = h.prove_keys(sks[:2], tapes=[bc.splice(k, off[j], on[j]) for j in range(2)])
    h.bank_fill(tapes=off)
    take0 = h.path_count(api.Kosk.PATH_BANK_TAKE)
    pi = C.create_string_buffer(b"\xa5" * (3 * h.proof_bytes), 3 * h.proof_bytes)
    ok = C.create_string_buffer(b"\x5a" * 3, 3)
    rc = lib.kosk_prove_keys_banked_batch(h._h, 3, b"".join(sks), b"".join(on), h.tape_bytes, None, 0, pi, ok)
    assert rc == -1
    assert "bank" in lib.kosk_last_error(h._h).decode()
    assert h.bank_level() == (2, bc.CAPACITY)
    assert pi.raw == b"\xa5" * (3 * h.proof_bytes) and ok.raw == b"\x5a" * 3
    assert h.path_count(api.Kosk.PATH_BANK_TAKE) == take0
    with pytest.raises(api.KoskError):
        h.stage_prover_keys_banked(sks, tapes=on)
    assert h.bank_level() == (2, bc.CAPACITY)
    got, okl = h.prove_keys_banked(sks[:2], tapes=on[:2])
    assert okl == [True, True]
    _same(got, want, ("after the refused call", k))
    # argument errors: both kinds of randomness, a short stride
    h.bank_fill(tapes=off[:1])
    assert lib.kosk_prove_keys_banked_batch(h._h, 1, sks[0], on[0], h.tape_bytes, bc.seed(k, 0), 32, pi, ok) == -1
    assert lib.kosk_prove_keys_banked_batch(h._h, 1, sks[0], on[0], h.tape_bytes - 1, None, 0, pi, ok) == -1
    assert lib.kosk_bank_fill(h._h, 1, on[0], h.tape_bytes, bc.seed(k, 0), 32) == -1
    assert h.bank_level() == (1, bc.CAPACITY)
    assert pi.raw == b"\xa5" * (3 * h.proof_bytes) and ok.raw == b"\x5a" * 3
    h.close()


@pytest.mark.parametrize("k", KS)
def test_a_rejected_key_consumes_its_entry(k, torch_cuda):
    n = 3
    h = _handle(k)
    sks = bc.sks(k, n)
    sks[1] = kc.pk_swapped(k)  # a record whose halves do not belong together: ok = 0
    off, on = [bc.tape(k, j, "off") for j in range(n)], [bc.tape(k, j, "on") for j in range(n)]
    want, want_ok = h.prove_keys(sks, tapes=[bc.splice(k, a, b) for a, b in zip(off, on)])
    assert want_ok == [True, False, True]
    h.bank_fill(tapes=off)
    got, ok = h.prove_keys_banked(sks, tapes=on)
    assert ok == want_ok
    assert got[1] == bytes(h.proof_bytes)
    _same(got, want, ("rejected key", k))
    assert h.bank_level() == (0, bc.CAPACITY)
    h.close()


@pytest.mark.parametrize("k", KS)
def test_armed_handle_makes_bound_proofs(k, torch_cuda):
    import hashlib
    api = _api()
    n = 2
    h = _handle(k)
    ctxs = [hashlib.sha3_256(b"kosk-bank-v1:context:%d:%d" % (k, i)).digest() for i in range(n)]
    sks, pks = bc.sks(k, n), bc.pks(k, n)
    off, on = [bc.tape(k, j, "off") for j in range(n)], [bc.tape(k, j, "on") for j in range(n)]
    plain, _ = h.prove_keys(sks, tapes=[bc.splice(k, a, b) for a, b in zip(off, on)])
    h.set_contexts(ctxs)
    want, _ = h.prove_keys(sks, tapes=[bc.splice(k, a, b) for a, b in zip(off, on)])
    h.bank_fill(tapes=off)
    got, ok = h.prove_keys_banked(sks, tapes=on)
    assert ok == [True] * n
    _same(got, want, ("armed", k))
    assert got[0] != plain[0]
    assert h.verify(got, pks) == [True] * n
    # the split call on host structs is still refused on an armed handle, with its text
    ib, rb, gb = api.lib.kosk_mlwe_inst_bytes(k), api.lib.kosk_randomness_bytes(k), api.lib.kosk_range_proof_bytes(k)
    pi = C.create_string_buffer(h.proof_bytes)
    assert api.lib.kosk_prove_prepared(h._h, 1, bytes(ib), bytes(rb), bytes(gb), on[0], h.tape_bytes, pi) == -1
    assert "no public key bytes to bind" in api.lib.kosk_last_error(h._h).decode()
    h.clear_contexts()
    assert h.verify(got, pks) == [False] * n  # under the context only
    h.close()


@pytest.mark.parametrize("k", KS)
def test_staging_form_and_a_packed_fetch(k, torch_cuda):
    api = _api()
    n = 3
    h = _handle(k)
    sks = bc.sks(k, n)
    off, on = [bc.tape(k, j, "off") for j in range(n)], [bc.tape(k, j, "on") for j in range(n)]
    assert h.stage_prover_keys(sks, tapes=[bc.splice(k, a, b) for a, b in zip(off, on)]) == [True] * n
    h.prove_resident(n)
    want = h.fetch_proofs_dense2(n)
    h.bank_fill(tapes=off)
    take0 = h.path_count(api.Kosk.PATH_BANK_TAKE)
    assert h.stage_prover_keys_banked(sks, tapes=on) == [True] * n
    assert h.bank_level() == (0, bc.CAPACITY) and h.path_count(api.Kosk.PATH_BANK_TAKE) == take0 + 1
    h.prove_resident(n)
    _same(h.fetch_proofs_dense2(n), want, ("staging form", k))
    # a wipe between staging and proving: refused as after any staging call
    h.bank_fill(tapes=off)
    h.stage_prover_keys_banked(sks, tapes=on)
    h.wipe_secrets()
    with pytest.raises(api.KoskError, match="staged inputs were wiped"):
        h.prove_resident(n)
    # and a non-banked staging call afterwards proves with the full front again
    assert h.stage_prover_keys(sks, tapes=[bc.splice(k, a, b) for a, b in zip(off, on)]) == [True] * n
    h.prove_resident(n)
    _same(h.fetch_proofs_dense2(n), want, ("full front after banked work", k))
    h.close()


@pytest.mark.parametrize("k", KS)
def test_entropy_modes_draw_the_sections(k, torch_cuda):
    """both NULL: tape mode draws M x 32 then (2M + 2KE) x 302 per entry at a fill and (3K + 4K eta1) x 302 per proof at a consuming call;
    seed mode one 32-byte draw per entry / proof"""
    import hashlib
    api = _api()
    n = 2
    h = _handle(k)
    M, E, eta1, T, O = bc.shape(k)
    sks = bc.sks(k, n)
    stream = hashlib.shake_256(b"kosk-bank-v1:entropy:%d" % k).digest(n * (T - 64))
    pos, sizes = [0], []

    def rb(nbytes):
        sizes.append(nbytes)
        out = stream[pos[0]:pos[0] + nbytes]
        pos[0] += nbytes
        return out
    h.set_randombytes(rb)
    h.bank_fill(n=n)
    assert sizes == ([32] * M + [302] * (2 * M + 2 * k * E)) * n
    cut = pos[0]
    del sizes[:]
    got, ok = h.prove_keys_banked(sks)
    assert sizes == [302] * ((3 * k + 4 * k * eta1) * n) and ok == [True] * n
    offl = [stream[b * (O - 64):(b + 1) * (O - 64)] for b in range(n)]
    onl = [stream[cut + b * (T - O):cut + (b + 1) * (T - O)] for b in range(n)]
    want, _ = h.prove_keys(sks, tapes=[bytes(64) + offl[b] + onl[b] for b in range(n)])
    _same(got, want, ("tape mode", k))
    h.set_entropy(api.ENTROPY_SEED)
    del sizes[:]
    pos[0] = 0
    h.bank_fill(n=n)
    got, ok = h.prove_keys_banked(sks)
    assert sizes == [32] * (2 * n)
    ta = [api.tape_from_seed(k, stream[32 * b:32 * b + 32]) for b in range(n)]
    tb = [api.tape_from_seed(k, stream[32 * (n + b):32 * (n + b) + 32]) for b in range(n)]
    want, _ = h.prove_keys(sks, tapes=[api.tape_splice(k, a, b) for a, b in zip(ta, tb)])
    _same(got, want, ("seed mode", k))
    h.set_randombytes(None)
    h.close()


@pytest.mark.parametrize("k", KS)
def test_key_generation_form(k, torch_cuda):
    """pk, sk and pi of the banked key generation = kosk_verifiable_keygen_batch on the spliced tapes; armed too; seeds too"""
    import hashlib
    api = _api()
    n = 3
    h = _handle(k)
    off, on = [bc.tape(k, j, "off") for j in range(n)], [bc.tape(k, j, "on") for j in range(n)]
    want = h.verifiable_keygen([bc.splice(k, a, b) for a, b in zip(off, on)])
    h.bank_fill(tapes=off)
    got = h.verifiable_keygen_banked(tapes=on)
    for what, g, w in zip(("pk", "sk", "pi"), got, want):
        _same(g, w, (what, k))
    assert h.verify(got[2], got[0]) == [True] * n and h.bank_level() == (0, bc.CAPACITY)
    SA, SB = [bc.seed(k, i, "a") for i in range(n)], [bc.seed(k, i, "b") for i in range(n)]
    want = h.verifiable_keygen([api.tape_splice(k, api.tape_from_seed(k, a), api.tape_from_seed(k, b)) for a, b in zip(SA, SB)])
    h.bank_fill(seeds=SA)
    got = h.verifiable_keygen_banked(seeds=SB)
    for what, g, w in zip(("pk", "sk", "pi"), got, want):
        _same(g, w, (what, "seeds", k))
    h.set_contexts([hashlib.sha3_256(b"kosk-bank-v1:kg-context:%d:%d" % (k, i)).digest() for i in range(n)])
    want = h.verifiable_keygen([bc.splice(k, a, b) for a, b in zip(off, on)])
    h.bank_fill(tapes=off)
    got = h.verifiable_keygen_banked(tapes=on)
    for what, g, w in zip(("pk", "sk", "pi"), got, want):
        _same(g, w, (what, "armed", k))
    assert h.verify(got[2], got[0]) == [True] * n
    h.close()


@pytest.mark.parametrize("k", KS)
def test_a_banked_proof_leaves_no_staged_inputs(k, torch_cuda):
    """The tape buffer never holds the offline sections of a banked proof and the rows of an entry serve one proof: after a banked key
    generation, a banked host-buffer call, and the one kosk_prove_resident behind a banked staging call, kosk_prove_resident is refused
    until a staging call has run -- it never runs a full front over other entries' offline bytes, and never a second proof on an entry"""
    api = _api()
    n = 2
    h = _handle(k)
    off, on = [bc.tape(k, j, "off") for j in range(4)], [bc.tape(k, j, "on") for j in range(4)]
    sks = bc.sks(k, 4)
    refused = "no resident prover inputs"
    # the sequence of concern: entries 0, 1 go out with other keys, entries 2, 3 make new keys at positions 0, 1, then a re-prove
    h.bank_fill(tapes=off)
    h.prove_keys_banked(sks[:n], tapes=on[:n])
    with pytest.raises(api.KoskError, match=refused):
        h.prove_resident(n)
    got = h.verifiable_keygen_banked(tapes=on[n:])
    before = h.fetch_proofs(n)
    assert before == got[2]
    with pytest.raises(api.KoskError, match=refused):
        h.prove_resident(n)
    assert h.fetch_proofs(n) == before  # nothing was proven
    # the staging form: one proof per staging call, also with another key's witness brought in between
    h.bank_fill(tapes=off[:n])
    assert h.stage_prover_keys_banked(sks[:n], tapes=on[:n]) == [True] * n
    h.prove_resident(n)
    first = h.fetch_proofs(n)
    h.witness_from_sk(sks[n:])
    with pytest.raises(api.KoskError, match=refused):
        h.prove_resident(n)
    assert h.fetch_proofs(n) == first
    # the non-banked calls keep their re-prove: same proof again
    want = h.verifiable_keygen([bc.splice(k, a, b) for a, b in zip(off[:n], on[:n])])
    h.stage_prover_keys(sks[:n], tapes=[bc.splice(k, a, b) for a, b in zip(off[:n], on[:n])])
    h.prove_resident(n)
    once = h.fetch_proofs(n)
    h.prove_resident(n)
    assert h.fetch_proofs(n) == once == first
    assert want[2] != once  # (other keys: the key generation's own)
    h.close()


@pytest.mark.parametrize("k", KS)
def test_tapes_in_device_memory(k, torch_cuda):
    """tapes in HBM: an aligned buffer (base and stride multiples of 8) is read in place, anything else goes section by section through a
    strided device copy; both on the fill's and on the consuming side, also for the key generation form"""
    torch = torch_cuda
    api = _api()
    lib = api.lib
    n = 3
    h = _handle(k)
    T = h.tape_bytes
    sks = bc.sks(k, n)
    off, on = [bc.tape(k, j, "off") for j in range(n)], [bc.tape(k, j, "on") for j in range(n)]
    spliced = [bc.splice(k, a, b) for a, b in zip(off, on)]
    want, _ = h.prove_keys(sks, tapes=spliced)
    want_kg = h.verifiable_keygen(spliced)

    def device(tapes, shift, stride):
        buf = bytearray(b"\xee" * (shift + n * stride + 8))
        for b, t in enumerate(tapes):
            buf[shift + b * stride:shift + b * stride + T] = t
        d = torch.frombuffer(buf, dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        assert d.data_ptr() % 8 == 0
        return d
    aligned = (T + 7) // 8 * 8
    for what, shift, stride in (("in place", 0, aligned), ("odd base", 1, aligned), ("odd stride", 0, aligned + 3)):
        d_off, d_on = device(off, shift, stride), device(on, shift, stride)
        pi, ok = C.create_string_buffer(n * h.proof_bytes), C.create_string_buffer(n)
        assert lib.kosk_bank_fill(h._h, n, C.c_void_p(d_off.data_ptr() + shift), stride, None, 0) == 0, what
        assert lib.kosk_prove_keys_banked_batch(h._h, n, b"".join(sks), C.c_void_p(d_on.data_ptr() + shift), stride, None, 0, pi, ok) == 0, what
        assert ok.raw == b"\x01" * n
        _same([pi.raw[b * h.proof_bytes:(b + 1) * h.proof_bytes] for b in range(n)], want, ("device tapes", what, k))
        pk, sk = C.create_string_buffer(n * h.pk_bytes), C.create_string_buffer(n * h.sk_bytes)
        assert lib.kosk_bank_fill(h._h, n, C.c_void_p(d_off.data_ptr() + shift), stride, None, 0) == 0, what
        assert lib.kosk_verifiable_keygen_banked_batch(h._h, n, C.c_void_p(d_on.data_ptr() + shift), stride, None, 0, pk, sk, pi) == 0, what
        assert pk.raw == b"".join(want_kg[0]) and sk.raw == b"".join(want_kg[1]) and pi.raw == b"".join(want_kg[2]), (what, k)
        del d_off, d_on
    assert h.bank_level() == (0, bc.CAPACITY)
    h.close()


@pytest.mark.parametrize("k", KS)
def test_key_generation_form_in_the_entropy_modes(k, torch_cuda):
    """both NULL at the key generation form: tape mode draws 64 bytes first, then (3K + 4K eta1) x 302, per proof; seed mode 32 bytes"""
    import hashlib
    api = _api()
    n = 2
    h = _handle(k)
    M, E, eta1, T, O = bc.shape(k)
    stream = hashlib.shake_256(b"kosk-bank-v1:kg-entropy:%d" % k).digest(n * T)
    pos, sizes = [0], []

    def rb(nbytes):
        sizes.append(nbytes)
        out = stream[pos[0]:pos[0] + nbytes]
        pos[0] += nbytes
        return out
    off = [bc.tape(k, j, "off") for j in range(n)]
    h.bank_fill(tapes=off)
    h.set_randombytes(rb)
    got = h.verifiable_keygen_banked(n=n)
    per = 64 + (T - O)
    assert sizes == ([64] + [302] * (3 * k + 4 * k * eta1)) * n and pos[0] == n * per
    drawn = [stream[b * per:(b + 1) * per] for b in range(n)]
    want = h.verifiable_keygen([drawn[b][:64] + off[b][64:O] + drawn[b][64:] for b in range(n)])
    for what, g, w in zip(("pk", "sk", "pi"), got, want):
        _same(g, w, (what, "tape mode", k))
    h.set_entropy(api.ENTROPY_SEED)
    del sizes[:]
    pos[0] = 0
    h.bank_fill(tapes=off)
    got = h.verifiable_keygen_banked(n=n)
    assert sizes == [32] * n
    tb = [api.tape_from_seed(k, stream[32 * b:32 * b + 32]) for b in range(n)]
    want = h.verifiable_keygen([api.tape_splice(k, a, b) for a, b in zip(off, tb)])
    for what, g, w in zip(("pk", "sk", "pi"), got, want):
        _same(g, w, (what, "seed mode", k))
    h.set_randombytes(None)
    h.close()


# ---- more than one handle: in a fresh child process (tests/gpu_child_bank.py), K = 2, 3, 4 inside
def test_erasure_of_the_bank(gpu_child, torch_cuda):
    out = gpu_child("from tests.gpu_child_bank import erasure; erasure()", timeout=300)
    assert out.count("erasure ok") == 3, out


def test_reserve_rules(gpu_child, torch_cuda):
    out = gpu_child("from tests.gpu_child_bank import reserve_rules; reserve_rules()", timeout=300)
    assert out.count("reserve_rules ok") == 3, out


def test_existing_calls_are_unaffected(gpu_child, torch_cuda):
    out = gpu_child("from tests.gpu_child_bank import existing_calls_unaffected; existing_calls_unaffected()", timeout=300)
    assert out.count("existing_calls_unaffected ok") == 3, out


def test_cohort_member_runs_banked_calls_on_its_own_block(gpu_child, torch_cuda):
    out = gpu_child("from tests.gpu_child_bank import cohort_member; cohort_member()", timeout=300)
    assert "cohort_member ok" in out, out


def test_bank_online_example(torch_cuda):
    """examples/bank_online.cpp on the C ABI: fill, banked proofs for kosk_kem_keypair_batch keys, verify"""
    import os
    import subprocess
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples", "bank_online")
    assert os.path.exists(exe), "examples/bank_online is built by __graft_entry__.build()"
    r = subprocess.run([exe, "3", "3"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0, r.stdout
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert lines and all(ln.endswith("= 1") for ln in lines), r.stdout
    assert lines[-1] == "[result] bank_online success = 1"
