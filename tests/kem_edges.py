"""The inputs of tests/golden/kem_edges_v1.json, shared by its generator (tests/golden/make_kem_edge_vectors.py) and the tests that
read it: the places where a Kyber KEM usually goes wrong.  Everything is derived from labels; the fixture holds results only.

Keys are kf.keypair(K, i) with indices of this file's own (HONEST, OTHER, the searched SAMPLING indices); random bytes are
SHAKE256("kosk-kem-edges-v1:" + label).

enc edges    a public key whose t-hat is 384 K bytes of one 12-bit value -- 0xFFF, 0, q - 1, q -- in front of an honest key's rho.
dec edges    the honest key's ciphertext CT = enc(pk_H, m_H) ("valid") and three foreign ones (all 0xFF, all 0x00, random bytes):
             s-hat of one value (0xFFF, 0, q - 1) x the four ciphertexts; the honest sk x the three foreign ones and x two
             ciphertexts that between them hold every d_u-bit and d_v-bit code (codes_ct); s-hat with every c < 767 stored as
             c + q (accepts); one bit of the stored H(pk) flipped; another key's pk || H(pk) || z behind the honest s-hat; another
             z with a tampered ciphertext.
sampling     keys whose rho drives rej_uniform (kyber/indcpa.c:124-145) through its rare ends, found by search over kf.keypair's
             indices (search(): the first index from SEARCH_FROM + 100 x the condition's number on that meets it), pinned in SAMPLING:
               a  some entry of A^T needs a fourth SHAKE128 block
               b  some entry takes its 256th coefficient from the last candidate of its third block
               c  some entry takes it from the first half of a 3-byte group whose second half is < q too (and must be dropped)
               d  every entry needs exactly three blocks
every byte   tamper_all(): bit at % 8 of byte at flipped, for every at of a ciphertext.
"""
import functools
import hashlib
import json
import os

from tests import kem_fixture as kf

Q = kf.Q
PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kem_edges_v1.json")
HONEST, OTHER = 131, 132  # kf.keypair indices past the 130 items of kem_vectors_v1.json
RHO_FROM = 133            # the enc edges take their rho from keys 133 .. 136
SEARCH_FROM = 1000
CONDS = ("a", "b", "c", "d")
# search(k, cond) for every K and condition: kf.keypair indices (tests/test_kem_edges_host.py checks the conditions on these keys)
SAMPLING = {2: {"a": 1015, "b": 1165, "c": 1200, "d": 1300}, 3: {"a": 1012, "b": 1109, "c": 1200, "d": 1300},
            4: {"a": 1010, "b": 1109, "c": 1200, "d": 1301}}
TAMPER_ITEM = 3           # the item of kem_vectors_v1.json (it stores its ct) whose every byte is tampered with
LAST_OF_THIRD_BLOCK = 3 * 112 - 1  # a SHAKE128 block is 56 groups of 3 bytes = 112 candidates


def rnd(label, n):
    return hashlib.shake_256(b"kosk-kem-edges-v1:" + label).digest(n)


def body_of(value, k):
    """384 K bytes that hold `value` in every 12-bit field (poly_tobytes, kyber/poly.c:128-147)"""
    return bytes([value & 0xFF, (value >> 8) | ((value & 0x0F) << 4), value >> 4]) * (128 * k)


BODIES = (("fff", 0xFFF), ("zero", 0), ("qm1", Q - 1), ("q", Q))
assert body_of(Q - 1, 2)[:3] == bytes.fromhex("000dd0") and body_of(Q, 2)[:3] == bytes.fromhex("011dd0") and body_of(0xFFF, 2)[:3] == b"\xff" * 3


def enc_edges(k):
    """[(name, pk, m)]"""
    return [("that_" + name, body_of(v, k) + kf.keypair(k, RHO_FROM + j)[0][-32:], rnd(b"m:%d:%s" % (k, name.encode()), 32))
            for j, (name, v) in enumerate(BODIES)]


def valid_input(k):
    """(pk_H, m_H): CT = enc of these is the valid ciphertext of the dec edges"""
    return kf.keypair(k, HONEST)[0], rnd(b"m:%d:valid" % k, 32)


def foreign_cts(k):
    n = kf.CT_BYTES[k]
    return [("ff", b"\xff" * n), ("00", bytes(n)), ("random", rnd(b"ct:%d" % k, n))]


def codes_ct(k, down):
    """a ciphertext whose u coefficients hold the d_u-bit codes 0, 1, 2 ... (down: 2^d_u - 1, 2^d_u - 2 ...) and whose v coefficients
    the d_v-bit codes likewise, mod 2^d: 256 K < 2^d_u <= 512 K, so the two directions together hold every code decompress can see
    (little-endian bit stream, polyvec_compress / poly_compress, kyber/polyvec.c:17-86, poly.c:19-81)"""
    du, dv = (11, 5) if k == 4 else (10, 4)
    out = b""
    for d, n in ((du, 256 * k), (dv, 256)):
        x = 0
        for i in range(n):
            x |= ((((1 << d) - 1 - i) if down else i) % (1 << d)) << (d * i)
        out += x.to_bytes(n * d // 8, "little")
    return out


def dec_edges(k, ct_valid):
    """[(name, ct, sk)] given CT = enc(*valid_input(k))"""
    sk = kf.keypair(k, HONEST)[1]
    pvb = 384 * k
    tail = sk[pvb:]
    assert len(ct_valid) == kf.CT_BYTES[k]
    out = []
    for name, v in BODIES[:3]:
        for cname, ct in [("valid", ct_valid)] + foreign_cts(k):
            out.append(("shat_%s:ct_%s" % (name, cname), ct, body_of(v, k) + tail))
    for cname, ct in foreign_cts(k) + [("codes_up", codes_ct(k, False)), ("codes_down", codes_ct(k, True))]:
        out.append(("honest:ct_" + cname, ct, sk))
    out.append(("shat_plus_q", ct_valid, kf.noncanonical_polyvec(sk[:pvb])[0] + tail))
    flipped = bytearray(sk)
    flipped[len(sk) - 64] ^= 1
    out.append(("stored_h_flip", ct_valid, bytes(flipped)))
    out.append(("foreign_pk_tail", ct_valid, sk[:pvb] + kf.keypair(k, OTHER)[1][pvb:]))
    out.append(("other_z:ct_tampered", tamper_bit(ct_valid, 7), sk[:-32] + rnd(b"z:%d" % k, 32)))
    return out


def tamper_bit(ct, at):
    t = bytearray(ct)
    t[at] ^= 1 << (at % 8)
    return bytes(t)


def tamper_all(ct):
    """one ciphertext per byte position: bit at % 8 of byte at flipped"""
    return [tamper_bit(ct, at) for at in range(len(ct))]


# ------------------------------------------------------------------------------------------------------- sampling --
def rho_of_seed(k, seed64):
    """kyber_keygen (kosk.cpp:12-14): buf[32] = K, hash_g over 33 bytes; the first half is the public seed"""
    return hashlib.sha3_512(seed64[:32] + bytes([k])).digest()[:32]


def entry_stats(rho, x, y):
    """rej_uniform (indcpa.c:124-145) over SHAKE128(rho || x || y), until 256 coefficients are accepted:
    (blocks squeezed, index of the candidate that became the 256th coefficient, whether the other half of its group is a dropped
    candidate < q -- only a first half can have one)"""
    buf = hashlib.shake_128(rho + bytes([x, y])).digest(168 * 12)
    ctr = 0
    for t in range(len(buf) // 3):
        b0, b1, b2 = buf[3 * t:3 * t + 3]
        d1, d2 = (b0 | (b1 << 8)) & 0xFFF, ((b1 >> 4) | (b2 << 4)) & 0xFFF
        if d1 < Q:
            ctr += 1
            if ctr == 256:
                return t // 56 + 1, 2 * t, d2 < Q
        if d2 < Q:
            ctr += 1
            if ctr == 256:
                return t // 56 + 1, 2 * t + 1, False
    raise AssertionError("12 blocks did not give 256 coefficients")


def matrix_stats(k, rho):
    """entry_stats of A^T[i][j] = XOF(rho, i, j) (gen_matrix transposed, indcpa.c:177-178), at index i K + j"""
    return [entry_stats(rho, i, j) for i in range(k) for j in range(k)]


def meets(cond, stats):
    if cond == "a":
        return any(s[0] == 4 for s in stats)
    if cond == "b":
        return any(s[1] == LAST_OF_THIRD_BLOCK for s in stats)
    if cond == "c":
        return any(s[1] % 2 == 0 and s[2] for s in stats)
    return all(s[0] == 3 for s in stats)


def search(k, cond):
    i = SEARCH_FROM + 100 * CONDS.index(cond)
    while not meets(cond, matrix_stats(k, rho_of_seed(k, kf.kg_seed(k, i)))):
        i += 1
    return i


def sampling_edges(k):
    """[(cond, kf.keypair index, m)]"""
    return [(c, SAMPLING[k][c], rnd(b"m:%d:sampling:%s" % (k, c.encode()), 32)) for c in CONDS]


@functools.lru_cache(maxsize=None)
def load():
    with open(PATH) as f:
        return json.load(f)
