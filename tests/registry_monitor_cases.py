"""Logs for the monitor's tests: valid ones made by registry_history_model.Log, and crafted ones with one known defect.
No GPU, no library: the host test runs them through the sequential model, the GPU test through kosk_monitor_feed."""
import hashlib
import random
import struct

from tests import registry_history_model as hm
from tests import registry_monitor_model as mm

ONES = b"\xff" * 32


def fp(tag):
    """a fingerprint: any 32 bytes"""
    return hashlib.sha3_256(b"registry-monitor:" + (tag if isinstance(tag, bytes) else str(tag).encode())).digest()


def checkpoint(log):
    return log.checkpoint(*mm.roots(log.k, log.capacity, log.table))


def scripted(k, capacity=8):
    """admit, admit over occupied slots, evict (with empty and repeated slots), an enrolment's admits, a checkpoint, two checkpoints in a
    row, and a checkpoint on the empty table"""
    log = hm.Log(k, capacity)
    log.admit([(0, fp(0)), (2, fp(1)), (5, fp(2))])
    log.admit([(2, fp(3)), (7, fp(4)), (0, fp(5))])
    log.evict([1, 2, 2, 5])
    log.admit([(1, fp(6)), (2, fp(7))])
    checkpoint(log)
    log.admit([(3, fp(8))])
    checkpoint(log)
    checkpoint(log)
    log.evict(list(range(capacity)))
    checkpoint(log)
    assert log.table == {} and struct.unpack("<I", log.events[-1][:4])[0] == hm.CHECKPOINT
    return log.events


def random_log(k, capacity, n, seed, cp_every=0, lo=0):
    """n events of a valid log: admits, evicts and admits over occupied slots at random (slots lo .. capacity - 1), a checkpoint as every
    cp_every-th event"""
    rng = random.Random(seed)
    log = hm.Log(k, capacity)
    while len(log.events) < n:
        if cp_every and len(log.events) % cp_every == cp_every - 1:
            checkpoint(log)
            continue
        s = rng.randrange(lo, capacity)
        if s in log.table and rng.random() < 0.5:
            log.evict([s])
        else:
            log.admit([(s, fp(b"r%d:%d" % (seed, len(log.events))))])
    return log.events[:n]  # a prefix of a valid log is one


def fill(k, capacity, slots, tag=b"fill"):
    """one ADMIT per slot, in the order given"""
    return [hm.record(hm.ADMIT, s, 0, fp(tag + b":%d" % s)) for s in slots]


def flip(rec, byte, bit=0):
    return rec[:byte] + bytes([rec[byte] ^ (1 << bit)]) + rec[byte + 1:]


def word(rec, at, value):
    return rec[:at] + struct.pack("<I", value) + rec[at + 4:]


def mutation_defects(k, capacity, events, i):
    """events with event i (an ADMIT or EVICT of a valid log) replaced so that it is the sole defect: [(name, events, reason)]"""
    table = mm.replay(k, capacity, events[:i])[3]
    ev = events[i]
    op = struct.unpack("<I", ev[:4])[0]
    assert op in (hm.ADMIT, hm.EVICT)
    out = [("op 0", word(ev, 0, 0), mm.BAD_RECORD), ("op 4", word(ev, 0, 4), mm.BAD_RECORD), ("op 2^31 + 1", word(ev, 0, 2 ** 31 + 1), mm.BAD_RECORD),
           ("word 12", flip(ev, 15, 7), mm.BAD_RECORD), ("b", flip(ev, 8), mm.BAD_RECORD), ("y first byte", flip(ev, 48), mm.BAD_RECORD),
           ("y last byte", flip(ev, 79, 7), mm.BAD_RECORD), ("slot == capacity", word(ev, 4, capacity), mm.BAD_SLOT),
           ("slot 2^32 - 1", word(ev, 4, 2 ** 32 - 1), mm.BAD_SLOT)]
    occupied = sorted(table)
    free = [s for s in range(capacity) if s not in table]
    if occupied:
        s = occupied[len(occupied) // 2]
        out.append(("admit occupied", hm.record(hm.ADMIT, s, 0, fp(b"late")), mm.ADMIT_OCCUPIED))
        out.append(("evict mismatch", hm.record(hm.EVICT, s, 0, flip(table[s], 31, 7)), mm.EVICT_MISMATCH))
    if free:
        out.append(("evict empty", hm.record(hm.EVICT, free[len(free) // 2], 0, fp(b"none")), mm.EVICT_EMPTY))
    return [(name, events[:i] + [rec] + events[i + 1:], why) for name, rec, why in out]


def checkpoint_defects(events, i):
    """events with checkpoint i altered in one place: [(name, events, reason)]"""
    ev = events[i]
    assert struct.unpack("<I", ev[:4])[0] == hm.CHECKPOINT
    out = [("word 12", flip(ev, 12), mm.BAD_RECORD), ("used", flip(ev, 4), mm.CP_USED), ("used high bit", flip(ev, 7, 7), mm.CP_USED),
           ("capacity", flip(ev, 8, 1), mm.CP_CAPACITY), ("slot_root first bit", flip(ev, 16), mm.CP_SLOT_ROOT), ("slot_root last bit", flip(ev, 47, 7), mm.CP_SLOT_ROOT),
           ("sorted_root first bit", flip(ev, 48), mm.CP_SORTED_ROOT), ("sorted_root last bit", flip(ev, 79, 7), mm.CP_SORTED_ROOT),
           ("used and both roots: the lowest reason", flip(flip(flip(ev, 4), 20), 60), mm.CP_USED),
           ("capacity and sorted_root", flip(flip(ev, 9), 70), mm.CP_CAPACITY)]
    return [(name, events[:i] + [rec] + events[i + 1:], why) for name, rec, why in out]
