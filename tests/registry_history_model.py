"""The registry history, format kosk-reghist-v1, restated in hashlib from the RECURSIVE definition alone: the tree over
the first n leaves is O for n = 0, the leaf for n = 1, and N(H(D[0:s]), H(D[s:n])) with s the largest power of two below n; an inclusion
path and a consistency proof are the recursions of RFC 6962.  Nothing here walks levels or set bits as the library's kernels and host
functions do, so agreement with them is agreement of two derivations.  The event rule of the mutating calls is restated as a table model
(class Log) that the GPU tests drive beside a handle."""
import hashlib
import struct

TAG = b"kosk-reghist-v1"
ADMIT, EVICT, CHECKPOINT = 1, 2, 3
EVENT_BYTES = 80
ZERO = bytes(32)


def _h(b):
    return hashlib.sha3_256(b).digest()


def event_leaf(k, h, op, slot): return _h(TAG + b"\x00" + h + struct.pack("<III", op, slot, k))
def checkpoint_leaf(k, slot_root, sorted_root, used, capacity): return _h(TAG + b"\x01" + slot_root + sorted_root + struct.pack("<III", used, capacity, k))
def node(l, r): return _h(TAG + b"\x02" + l + r)
def empty(k): return _h(TAG + b"\x03" + struct.pack("<I", k))


# the six digests of INTEGRATION.md 8.7
PINS = {
    "O2": "d8a55b610cc5228141b2f211b388d4bfc4c5aea61aa6496c031c1be6b52acbfb",
    "O3": "3bbed6e89d035147e6e7ad59edb52a42a5610bd4b48ac5f302f713848ebe91f3",
    "O4": "5aa09ad7d3d4c522d1ec3cbcdcc9ed83ad4f6e72f618a5a3f2b0156266a8ae9e",
    "V": "a072946f099b63a9511d962e7ec11810ff0170e9188caa33afe7ef116fa8f989",
    "C": "c3ac69cab994754912dc117aab3f76ccc0047ff5af0207138ac8aa4228f221f8",
    "N": "a94fdaf8f5573f9a257629c4d09419ae82d0d3bcfe77ab04f1f947cf628ca528",
}


def record(op, a, b=0, x=ZERO, y=ZERO):
    """the stored event record"""
    return struct.pack("<IIII", op, a, b, 0) + x + y


def leaf(k, rec):
    """the leaf of a stored event record; None where the library refuses it"""
    op, a, b, z = struct.unpack("<IIII", rec[:16])
    x, y = rec[16:48], rec[48:80]
    if k not in (2, 3, 4) or len(rec) != EVENT_BYTES or z or op not in (ADMIT, EVICT, CHECKPOINT):
        return None
    if op == CHECKPOINT:
        return checkpoint_leaf(k, x, y, a, b)
    if b or y != ZERO:
        return None
    return event_leaf(k, x, op, a)


def depth(n):
    if n < 0:
        return -1
    d = 0
    while (1 << d) < n:
        d += 1
    return d


def path_bytes(n): return 16 + 32 * depth(n) if n >= 1 else 0
def consistency_bytes(n): return 16 + 32 * (depth(n) + 1) if n >= 1 else 0


def _split(n):
    s = 1
    while 2 * s < n:
        s *= 2
    return s


def mth(k, leaves):
    """H(D[0:n])"""
    n = len(leaves)
    if n == 0:
        return empty(k)
    if n == 1:
        return leaves[0]
    s = _split(n)
    return node(mth(k, leaves[:s]), mth(k, leaves[s:]))


def path(k, i, leaves):
    """the audit path of leaf i, lowest level first"""
    n = len(leaves)
    if n == 1:
        return []
    s = _split(n)
    if i < s:
        return path(k, i, leaves[:s]) + [mth(k, leaves[s:])]
    return path(k, i - s, leaves[s:]) + [mth(k, leaves[:s])]


def _sub(k, m, leaves, whole):
    n = len(leaves)
    if m == n:
        return [] if whole else [mth(k, leaves)]
    s = _split(n)
    if m <= s:
        return _sub(k, m, leaves[:s], whole) + [mth(k, leaves[s:])]
    return _sub(k, m - s, leaves[s:], False) + [mth(k, leaves[:s])]


def proof(k, m, leaves):
    """the consistency proof from the first m leaves to all of them; empty for m == 0 and m == n"""
    return _sub(k, m, leaves, True) if 0 < m < len(leaves) else []


def pack(items, w1, size, bound):
    """a proof record: the header, the items, zero padding up to `bound` items"""
    assert len(items) <= bound
    return struct.pack("<IIII", len(items), w1, size, 0) + b"".join(items) + bytes(32 * (bound - len(items)))


def inclusion_record(k, i, leaves): return pack(path(k, i, leaves), i, len(leaves), depth(len(leaves)))
def consistency_record(k, m, leaves): return pack(proof(k, m, leaves), m, len(leaves), depth(len(leaves)) + 1)


class Log:
    """the table and the event list that the event rule of INTEGRATION.md 8.7 produces, call by call"""

    def __init__(self, k, capacity):
        self.k, self.capacity = k, capacity
        self.table = {}   # slot -> fingerprint
        self.events = []  # stored records

    def admit(self, pairs):
        """pairs: (slot, fingerprint) of the ACCEPTED positions in ascending position"""
        for slot, _ in pairs:
            if slot in self.table:
                self.events.append(record(EVICT, slot, 0, self.table[slot]))
        for slot, h in pairs:
            self.events.append(record(ADMIT, slot, 0, h))
            self.table[slot] = h

    def evict(self, slots):
        for slot in slots:
            if slot in self.table:
                self.events.append(record(EVICT, slot, 0, self.table.pop(slot)))

    def checkpoint(self, slot_root, sorted_root):
        self.events.append(record(CHECKPOINT, len(self.table), self.capacity, slot_root, sorted_root))
        return len(self.events) - 1

    def leaves(self, n=None):
        return [leaf(self.k, e) for e in self.events[:n]]


def replay(events):
    """the (slot -> fingerprint) table that events give on an empty one"""
    table = {}
    for e in events:
        op, a = struct.unpack("<II", e[:8])
        if op == ADMIT:
            assert a not in table
            table[a] = e[16:48]
        elif op == EVICT:
            assert table.pop(a) == e[16:48]
    return table
