"""The registry monitor's replay rule as a SEQUENTIAL replay with verdicts: one event after the other onto a dict, every
check in the order of the text, the first failure returned.  Nothing here sorts events, looks at neighbours or works in segments as the
library's kernels do, so agreement with them is agreement of two derivations.  Built on registry_history_model (records and leaves),
registry_tree_model and registry_sorted_model (the two state roots) only."""
import struct

from tests import registry_history_model as hm
from tests import registry_sorted_model as sm
from tests import registry_tree_model as tm

OK, BAD_RECORD, BAD_SLOT, ADMIT_OCCUPIED, EVICT_EMPTY, EVICT_MISMATCH, CP_USED, CP_CAPACITY, CP_SLOT_ROOT, CP_SORTED_ROOT = range(10)
NAMES = ["OK", "BAD_RECORD", "BAD_SLOT", "ADMIT_OCCUPIED", "EVICT_EMPTY", "EVICT_MISMATCH", "CP_USED", "CP_CAPACITY", "CP_SLOT_ROOT", "CP_SORTED_ROOT"]
ZERO = bytes(32)


def slot_root(k, capacity, table):
    """the slot tree's root of {slot: h}: only the nodes that differ from the all-empty tree are hashed"""
    lv, blank = tm.sparse_root(k, capacity, table)
    return lv[-1].get(0, blank[-1])


def sorted_root(k, capacity, table):
    """the sorted tree's root of {slot: h}: the entries' leaves, and one all-padding node per level beside them"""
    d = tm.depth(capacity)
    cur = [sm.leaf(k, h, s) for h, s in sm.entries(table)]
    blank = sm.pad(k)
    for _ in range(d):
        if len(cur) % 2:
            cur.append(blank)
        cur = [sm.node(cur[2 * i], cur[2 * i + 1]) for i in range(len(cur) // 2)]
        blank = sm.node(blank, blank)
    return cur[0] if cur else blank


def roots(k, capacity, table):
    return slot_root(k, capacity, table), sorted_root(k, capacity, table)


def verdict(k, capacity, table, rec):
    """the lowest-numbered reason why the stored record `rec` is invalid on `table` ({slot: h}), or OK"""
    op, a, b, z = struct.unpack("<IIII", rec[:16])
    x, y = rec[16:48], rec[48:80]
    if op not in (hm.ADMIT, hm.EVICT, hm.CHECKPOINT) or z:
        return BAD_RECORD
    if op == hm.CHECKPOINT:
        if a != len(table):
            return CP_USED
        if b != capacity:
            return CP_CAPACITY
        if x != slot_root(k, capacity, table):
            return CP_SLOT_ROOT
        if y != sorted_root(k, capacity, table):
            return CP_SORTED_ROOT
        return OK
    if b or y != ZERO:
        return BAD_RECORD
    if a >= capacity:
        return BAD_SLOT
    if op == hm.ADMIT:
        return ADMIT_OCCUPIED if a in table else OK
    if a not in table:
        return EVICT_EMPTY
    return OK if table[a] == x else EVICT_MISMATCH


def replay(k, capacity, events, table=None):
    """events onto `table` (a copy of it; default: empty) -> (ok, bad_index, reason, table, size).  Accepted: (True, -1, OK, the table after
    all events, len(events)).  Rejected: (False, the index of the lowest invalid event, its lowest reason, the table of the events before
    it, that index)"""
    table = dict(table or {})
    for i, rec in enumerate(events):
        why = verdict(k, capacity, table, rec)
        if why != OK:
            return False, i, why, table, i
        op, a = struct.unpack("<II", rec[:8])
        if op == hm.ADMIT:
            table[a] = rec[16:48]
        elif op == hm.EVICT:
            del table[a]
    return True, -1, OK, table, len(events)


def checkpoint(k, capacity, table):
    """the checkpoint record a registrar appends on `table`"""
    return hm.record(hm.CHECKPOINT, len(table), capacity, *roots(k, capacity, table))
