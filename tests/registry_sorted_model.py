"""The sorted tree, format kosk-regsort-v1, in hashlib: the three hashes, the sorted entries of a registry's content,
every level of the tree over them, the rank of a query, the proof record the registrar gives and the verifier that reads it.  The three
padding leaves and S(00^32, 0) for k = 3 are pinned in full."""
import bisect
import hashlib
import struct

from tests.registry_tree_model import depth

TAG = b"kosk-regsort-v1"
assert len(TAG) == 15

# Z for kyber_k 2, 3, 4: SHA3-256(TAG || 01 || LE32(k))
PAD = {
    2: bytes.fromhex("becb0cab467ebf22bfdba3f689f2f5c073785571975013ed08a36f92fc367cf1"),
    3: bytes.fromhex("4681eaa29349e1b455d902e2fbfdd7fda743ab7db289ea704dd533faf9186bf2"),
    4: bytes.fromhex("d8d33b6a86723fba711677b6d1fefe8be3f2fd3fb548179cf20d3b79c35d9ed7"),
}
# S(00^32, 0) for kyber_k 3
LEAF_ZERO_K3 = bytes.fromhex("0f9fbb3cb7e02ac0ce0b815b6ec6cc29edd6595605393f3b604968eede04d643")

NEITHER, ABSENT, PRESENT = 0, 1, 2
FLAG_LEFT, FLAG_RIGHT, FLAG_RIGHT_KEY, FLAG_PRESENT = 1, 2, 4, 8


def leaf(k, h, slot):
    """S(h, slot): the leaf of the entry (h, slot)"""
    assert len(h) == 32 and slot >= 0
    return hashlib.sha3_256(TAG + b"\x00" + h + slot.to_bytes(4, "little") + k.to_bytes(4, "little")).digest()


def pad(k):
    """Z: the leaf of every position behind the entries"""
    return hashlib.sha3_256(TAG + b"\x01" + k.to_bytes(4, "little")).digest()


def node(left, right):
    assert len(left) == 32 and len(right) == 32
    return hashlib.sha3_256(TAG + b"\x02" + left + right).digest()


def proof_bytes(d):
    return 16 + 64 + 64 * d if 0 <= d <= 31 else 0


def entries(content):
    """content: {slot: h} of the occupied slots -> [(h, slot)] ascending by h (bytes order), then slot"""
    return sorted((h, s) for s, h in content.items())


def levels(k, capacity, content):
    """every level of the sorted tree, level 0 (2^D leaves) first"""
    d = depth(capacity)
    ent = entries(content)
    assert len(ent) <= capacity
    z = pad(k)
    out = [[leaf(k, *ent[i]) if i < len(ent) else z for i in range(1 << d)]]
    for _ in range(d):
        below = out[-1]
        out.append([node(below[2 * i], below[2 * i + 1]) for i in range(len(below) // 2)])
    return out


def root(lv):
    return lv[-1][0]


def path(lv, pos):
    return b"".join(lv[l][(pos >> l) ^ 1] for l in range(len(lv) - 1))


def root_from_path(k, d, pos, h, slot, p):
    """the root that position pos, its entry (h None: padding) and the path imply"""
    assert len(p) == 32 * d and 0 <= pos < (1 << d)
    cur = pad(k) if h is None else leaf(k, h, slot)
    for l in range(d):
        sib = p[32 * l:32 * l + 32]
        cur = node(sib, cur) if (pos >> l) & 1 else node(cur, sib)
    return cur


def rank(ent, x):
    """(lb, present): the number of entries with h < x, and whether entry lb holds x"""
    lb = bisect.bisect_left(ent, (x, -1))
    return lb, lb < len(ent) and ent[lb][0] == x


def record(pos_l, slot_l, slot_r, flags, h_l, h_r, path_l, path_r):
    return struct.pack("<iiiI", pos_l, slot_l, slot_r, flags) + h_l + h_r + path_l + path_r


def prove(k, capacity, content, x, lv=None):
    """(kind, record) for query x, as kosk_registry_prove_absent gives them"""
    d = depth(capacity)
    ent = entries(content)
    lv = lv or levels(k, capacity, content)
    lb, present = rank(ent, x)
    zero, nopath = bytes(32), bytes(32 * d)
    if present:
        return PRESENT, record(lb, ent[lb][1], 0, FLAG_LEFT | FLAG_PRESENT, x, zero, path(lv, lb), nopath)
    left, right, key = lb >= 1, lb < (1 << d), lb < len(ent)
    return ABSENT, record(lb - 1 if left else -1, ent[lb - 1][1] if left else 0, ent[lb][1] if key else 0,
                          (FLAG_LEFT if left else 0) | (FLAG_RIGHT if right else 0) | (FLAG_RIGHT_KEY if key else 0),
                          ent[lb - 1][0] if left else zero, ent[lb][0] if key else zero,
                          path(lv, lb - 1) if left else nopath, path(lv, lb) if right else nopath)


def check(k, d, x, rec, rt):
    """the verifier: PRESENT, ABSENT or NEITHER"""
    assert len(rec) == proof_bytes(d) and len(x) == 32 and len(rt) == 32
    pos_l, slot_l, slot_r, flags = struct.unpack("<iiiI", rec[:16])
    h_l, h_r, path_l, path_r = rec[16:48], rec[48:80], rec[80:80 + 32 * d], rec[80 + 32 * d:]
    p = 1 << d

    def walks(pos, h, slot, pth):
        return 0 <= pos < p and (h is None or slot >= 0) and root_from_path(k, d, pos, h, slot, pth) == rt

    if flags == FLAG_LEFT | FLAG_PRESENT:
        return PRESENT if h_l == x and walks(pos_l, h_l, slot_l, path_l) else NEITHER
    left, right, key = bool(flags & FLAG_LEFT), bool(flags & FLAG_RIGHT), bool(flags & FLAG_RIGHT_KEY)
    if flags & ~7 or not (left or right) or (key and not right):
        return NEITHER
    if left:
        if not (h_l < x and walks(pos_l, h_l, slot_l, path_l)):
            return NEITHER
    elif pos_l != -1:
        return NEITHER
    if right:
        if pos_l + 1 >= p:
            return NEITHER
        if not (x < h_r and walks(pos_l + 1, h_r, slot_r, path_r) if key else walks(pos_l + 1, None, 0, path_r)):
            return NEITHER
    elif pos_l != p - 1:
        return NEITHER
    return ABSENT


def neighbours(h):
    """h - 1 and h + 1 as 32-byte big-endian numbers, where they exist"""
    v = int.from_bytes(h, "big")
    return [(v + dv).to_bytes(32, "big") for dv in (-1, 1) if 0 <= v + dv < 1 << 256]
