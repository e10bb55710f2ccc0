"""The registry tree, format kosk-regtree-v1, in hashlib: the three hashes, the depth, every level of the tree over a
registry's content, the path of a slot and the walk from a leaf up to the root.  The three empty leaves are pinned in full."""
import hashlib

TAG = b"kosk-regtree-v1"
assert len(TAG) == 15

# E for kyber_k 2, 3, 4: SHA3-256(TAG || 01 || LE32(k))
EMPTY = {
    2: bytes.fromhex("2aca555fb51e71bf9d3f07884d94a971cde10c45bb998bf8b5d1f7a142f3f0a6"),
    3: bytes.fromhex("dd6d2c3c4508f2e7e2c9546892161d7d5cc274b71bd91d14d98a49fc6ae0c8b1"),
    4: bytes.fromhex("a93686a2334041d2f8e3689e2cbb39e0b710b31e0454287f441c4aebdea29566"),
}


def leaf(k, h):
    """L(h): the leaf of an occupied slot whose stored SHA3-256(pk) is h"""
    assert len(h) == 32
    return hashlib.sha3_256(TAG + b"\x00" + h + k.to_bytes(4, "little")).digest()


def empty(k):
    """E: the leaf of an empty slot and of every padding position"""
    return hashlib.sha3_256(TAG + b"\x01" + k.to_bytes(4, "little")).digest()


def node(left, right):
    assert len(left) == 32 and len(right) == 32
    return hashlib.sha3_256(TAG + b"\x02" + left + right).digest()


def depth(capacity):
    """the smallest D with 2^D >= capacity; -1 for capacity < 1"""
    if capacity < 1:
        return -1
    d = 0
    while (1 << d) < capacity:
        d += 1
    return d


def tree_bytes(capacity):
    return 0 if capacity < 1 else 32 * (2 * (1 << depth(capacity)) - 1)


def levels(k, capacity, content):
    """every level of the tree, level 0 (2^D leaves) first; content: {slot: h} of the occupied slots"""
    d = depth(capacity)
    assert all(0 <= s < capacity for s in content)
    e = empty(k)
    out = [[leaf(k, content[s]) if s in content else e for s in range(1 << d)]]
    for _ in range(d):
        below = out[-1]
        out.append([node(below[2 * i], below[2 * i + 1]) for i in range(len(below) // 2)])
    return out


def root(lv):
    return lv[-1][0]


def path(lv, slot):
    """the D sibling records of `slot`, level 0 first, as one bytes"""
    return b"".join(lv[l][(slot >> l) ^ 1] for l in range(len(lv) - 1))


def root_from_path(k, d, slot, h, p):
    """the root that slot, h (None: the slot is empty) and the path imply"""
    assert len(p) == 32 * d and 0 <= slot < (1 << d)
    cur = empty(k) if h is None else leaf(k, h)
    for l in range(d):
        sib = p[32 * l:32 * l + 32]
        cur = node(sib, cur) if (slot >> l) & 1 else node(cur, sib)
    return cur


def sparse_root(k, capacity, content):
    """the root and the paths' material for a LARGE capacity without 2^D hashes: {level: {index: node}} of the nodes that differ from the
    all-empty tree, and the list of all-empty nodes per level"""
    d = depth(capacity)
    blank = [empty(k)]
    for _ in range(d):
        blank.append(node(blank[-1], blank[-1]))
    lv = [{s: leaf(k, h) for s, h in content.items()}]
    for l in range(d):
        up = {}
        for i in {s >> 1 for s in lv[l]}:
            up[i] = node(lv[l].get(2 * i, blank[l]), lv[l].get(2 * i + 1, blank[l]))
        lv.append(up)
    return lv, blank


def sparse_path(lv, blank, slot):
    return b"".join(lv[l].get((slot >> l) ^ 1, blank[l]) for l in range(len(lv) - 1))
