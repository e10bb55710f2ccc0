"""The model of the registry's fingerprint index: a dict from fingerprint to sorted slots, the enrol rule, the home
formula, and keys ground onto chosen home entries.  kosk_registry_admit makes no encoding check, so any bytes of the right length are a
key; a fingerprint is hashlib's SHA3-256 of them."""
import hashlib

REJECTED, ADMITTED, DUPLICATE = 0, 1, 2


def fp(pk):
    return hashlib.sha3_256(pk).digest()


def entries(capacity):
    """T: the smallest power of two >= 2 x capacity; 0 for capacity < 1"""
    if capacity < 1:
        return 0
    t = 2
    while t < 2 * capacity:
        t *= 2
    return t


def home(capacity, h):
    """LE32(h[0..4)) & (T - 1)"""
    return int.from_bytes(h[:4], "little") & (entries(capacity) - 1)


def grind(capacity, target_home, count, size, tag=b""):
    """`count` distinct byte strings of `size` bytes (a pk record) whose fingerprint's home is target_home; tag separates the families"""
    out, i = [], 0
    while len(out) < count:
        pk = hashlib.shake_256(b"registry-grind:%d:%d:%d:" % (capacity, target_home, i) + tag).digest(size)
        if home(capacity, fp(pk)) == target_home:
            out.append(pk)
        i += 1
    return out


class Model:
    def __init__(self, capacity):
        self.capacity = capacity
        self.slots = [None] * capacity  # slot -> pk bytes

    def table(self):
        """fingerprint -> sorted slots"""
        t = {}
        for s, pk in enumerate(self.slots):
            if pk is not None:
                t.setdefault(fp(pk), []).append(s)
        return t

    def find(self, h):
        return self.table().get(h, [-1])[0]

    def admit(self, pks, slots, accept=None):
        for b, (pk, s) in enumerate(zip(pks, slots)):
            if accept is None or accept[b]:
                self.slots[s] = pk

    def evict(self, slots):
        for s in slots:
            self.slots[s] = None

    def enrol(self, pks, accept=None):
        """-> (slots, status), or None when the registry is full (nothing changed)"""
        new, table = list(self.slots), self.table()
        given, slots, status = {}, [], []
        free = (s for s in range(self.capacity) if self.slots[s] is None)
        for b, pk in enumerate(pks):
            h = fp(pk)
            if accept is not None and not accept[b]:
                slots.append(-1); status.append(REJECTED)
            elif h in table or h in given:
                slots.append(table[h][0] if h in table else given[h]); status.append(DUPLICATE)
            else:
                s = next(free, None)
                if s is None:
                    return None
                given[h] = s; new[s] = pk
                slots.append(s); status.append(ADMITTED)
        self.slots = new
        return slots, status
