"""kosk-headsig-v1 in hashlib alone, written from the format text: key generation, signing and verification of the
registrar's signature over a history head.  Winternitz chains (w = 8, 34 chains of 255 steps) under a Merkle tree of 2^h one-time keys,
every hash SHAKE256 with 32 bytes of output; u32 / u16 / u8 are big-endian, the records' headers little-endian."""
import hashlib
import struct

P = 34
STEPS = 255
PUB_BYTES = 52
TAG = b"kosk-sighead-v1"


def H(x):
    return hashlib.shake_256(x).digest(32)


def u32(x):
    return struct.pack(">I", x)


def u16(x):
    return struct.pack(">H", x)


def u8(x):
    return struct.pack(">B", x)


def sig_bytes(h):
    return 16 + 32 + P * 32 + 32 * h if 1 <= h <= 24 else 0


def statement(k, root, size):
    assert len(root) == 32
    return TAG + b"\x00" + root + struct.pack("<II", size, k)


def x_start(I, q, i, seed):
    return H(I + u32(q) + u16(i) + u8(0xFF) + seed)


def randomizer(I, q, seed):
    return H(I + u32(q) + u16(0xFFFD) + u8(0xFF) + seed)


def chain(I, q, i, t, first, last):
    """t through steps j = first .. last - 1"""
    for j in range(first, last):
        t = H(I + u32(q) + u16(i) + u8(j) + t)
    return t


def ots_public(I, q, ys):
    return H(I + u32(q) + u16(0x8080) + b"".join(ys))


def leaf(I, h, q, K):
    return H(I + u32((1 << h) + q) + u16(0x8282) + K)


def node(I, r, left, right):
    return H(I + u32(r) + u16(0x8383) + left + right)


def digest(I, q, C, S):
    return H(I + u32(q) + u16(0x8181) + C + S)


def coefficients(Q):
    a = list(Q)
    cks = sum(255 - v for v in a)
    return a + [cks >> 8, cks & 255]


class Key:
    """every node of the tree of (h, seed, I): T[r] for r = 1 .. 2^(h+1) - 1"""

    def __init__(self, h, seed, I):
        assert 1 <= h <= 24 and len(seed) == 32 and len(I) == 16
        self.h, self.seed, self.I = h, seed, I
        T = [None] * (2 << h)
        for q in range(1 << h):
            ys = [chain(I, q, i, x_start(I, q, i, seed), 0, STEPS) for i in range(P)]
            T[(1 << h) + q] = leaf(I, h, q, ots_public(I, q, ys))
        for r in range((1 << h) - 1, 0, -1):
            T[r] = node(I, r, T[2 * r], T[2 * r + 1])
        self.T = T
        self.pub = struct.pack("<I", h) + I + T[1]

    def sign(self, k, root, size, seen=None):
        """the signature of the head (root, size) with leaf q = size; seen: a set that collects the coefficients"""
        h, I, q = self.h, self.I, size
        assert 0 <= q < (1 << h)
        C = randomizer(I, q, self.seed)
        a = coefficients(digest(I, q, C, statement(k, root, size)))
        if seen is not None:
            seen.update(a)
        z = [chain(I, q, i, x_start(I, q, i, self.seed), 0, a[i]) for i in range(P)]
        path = [self.T[(((1 << h) + q) >> l) ^ 1] for l in range(h)]
        return struct.pack("<IIII", h, q, 0, 0) + C + b"".join(z) + b"".join(path)


def verify(pub, k, root, size, sig):
    """True / False; None for the arguments the host function refuses (-1)"""
    if len(pub) != PUB_BYTES or k not in (2, 3, 4) or len(root) != 32 or size < 0:
        return None
    h = struct.unpack("<I", pub[:4])[0]
    if not 1 <= h <= 24:
        return None
    I, top = pub[4:20], pub[20:52]
    assert len(sig) == sig_bytes(h)
    sh, q, r0, r1 = struct.unpack("<IIII", sig[:16])
    if sh != h or q != size or q >= (1 << h) or r0 or r1:
        return False
    C = sig[16:48]
    a = coefficients(digest(I, q, C, statement(k, root, size)))
    ys = [chain(I, q, i, sig[48 + 32 * i:80 + 32 * i], a[i], STEPS) for i in range(P)]
    cur = leaf(I, h, q, ots_public(I, q, ys))
    r = (1 << h) + q
    for l in range(h):
        sib = sig[48 + 32 * P + 32 * l:80 + 32 * P + 32 * l]
        cur = node(I, r // 2, sib, cur) if r & 1 else node(I, r // 2, cur, sib)
        r //= 2
    return cur == top


def coefficients_of(pub, k, root, size, sig):
    """a[] as the verifier sees it (the header is taken as valid)"""
    return coefficients(digest(pub[4:20], size, sig[16:48], statement(k, root, size)))


# ---- the tampers of the CPU list, each the sole defect; (name, function(pub, root, size, sig) -> (pub, root, size, sig)) ----
def _flip(b, at, bit=0):
    b = bytearray(b)
    b[at] ^= 1 << bit
    return bytes(b)


def tampers(h):
    zoff, poff = 48, 48 + 32 * P
    t = [("C bit", lambda p, r, s, g: (p, r, s, _flip(g, 16 + 5, 3)))]
    for i in (0, 31, 32, 33):
        t.append(("z[%d] bit" % i, lambda p, r, s, g, i=i: (p, r, s, _flip(g, zoff + 32 * i + 7, 1))))
    t.append(("path level 0 bit", lambda p, r, s, g: (p, r, s, _flip(g, poff + 3, 6))))
    t.append(("path level h-1 bit", lambda p, r, s, g: (p, r, s, _flip(g, poff + 32 * (h - 1) + 31, 7))))
    t.append(("root bit", lambda p, r, s, g: (p, _flip(r, 17, 2), s, g)))
    t.append(("I bit", lambda p, r, s, g: (_flip(p, 4 + 9, 4), r, s, g)))
    t.append(("T[1] bit", lambda p, r, s, g: (_flip(p, 20 + 30, 0), r, s, g)))
    t.append(("q != size", lambda p, r, s, g: (p, r, s ^ 1, g)))
    t.append(("header h differs", lambda p, r, s, g: (p, r, s, struct.pack("<I", h + 1) + g[4:])))
    t.append(("q = 2^h", lambda p, r, s, g: (p, r, 1 << h, g[:4] + struct.pack("<I", 1 << h) + g[8:])))
    t.append(("reserved word 0", lambda p, r, s, g: (p, r, s, g[:8] + struct.pack("<I", 1) + g[12:])))
    t.append(("reserved word 1", lambda p, r, s, g: (p, r, s, g[:12] + struct.pack("<I", 1 << 31) + g[16:])))
    return t


def advance_forgery(pub, k, root, size, sig, i):
    """z[i] taken one step further, as a forger who wants a larger a[i] would, with the checksum chains left as they are; None where
    a[i] = 255 (no step is left)"""
    I = pub[4:20]
    a = coefficients_of(pub, k, root, size, sig)
    if a[i] >= STEPS:
        return None
    z = chain(I, size, i, sig[48 + 32 * i:80 + 32 * i], a[i], a[i] + 1)
    return sig[:48 + 32 * i] + z + sig[80 + 32 * i:]
