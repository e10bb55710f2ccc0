"""Shared by the tests of the offline bank (tests/test_bank_host.py, tests/test_gpu_31_bank.py, tests/gpu_child_bank.py):
the sizes every GPU case uses, deterministic tapes and seeds, the tape formula restated, and the splice.  Keys come from
tests/keyproof_cases.py.  Nothing here is modified by a test."""
import functools
import hashlib

from tests import keyproof_cases as kc

KS = kc.KS
MAX_BATCH = 4
CAPACITY = 6
RS_COLUMNS = 1710  # evaluation points of a sharing: the least an entry can store per row


def shape(k):
    """(M, E, eta1, T, O): M = 71 + 2K, E = 2 eta1 + 1, T = kosk_tape_bytes, O = end of the offline section"""
    eta1 = kc.ETA1[k]
    M, E = 71 + 2 * k, 2 * eta1 + 1
    T = 64 + 32 * M + 302 * (2 * M + 2 * k * E + 3 * k + 4 * k * eta1)
    O = 64 + 32 * M + 302 * (2 * M + 2 * k * E)
    return M, E, eta1, T, O


def sections(k):
    """[(offset, size)] of the three sections by the formula of the issue, not by the library"""
    _M, _E, _eta1, T, O = shape(k)
    return [(0, 64), (64, O - 64), (O, T - O)]


@functools.lru_cache(maxsize=None)
def tape(k, i, tag="a"):
    return hashlib.shake_256(b"kosk-bank-v1:tape:%d:%d:%s" % (k, i, tag.encode())).digest(shape(k)[3])


def seed(k, i, tag="a"):
    return hashlib.shake_256(b"kosk-bank-v1:seed:%d:%d:%s" % (k, i, tag.encode())).digest(32)


def splice(k, offline_tape, online_tape, head=None):
    """key seed (of `head`, default the online tape) || offline section of offline_tape || online section of online_tape"""
    (o0, s0), (o1, s1), (o2, s2) = sections(k)
    head = online_tape if head is None else head
    return head[o0:o0 + s0] + offline_tape[o1:o1 + s1] + online_tape[o2:o2 + s2]


def sks(k, n, first=0):
    return [kc.honest(k, first + i)[1] for i in range(n)]


def pks(k, n, first=0):
    return [kc.honest(k, first + i)[0] for i in range(n)]


def offline_compact(k, t):
    """the offline section as kosk_prepare_randomness takes it: the M seeds, then the 2M slices of the f / NTT f sharings"""
    M = shape(k)[0]
    return t[64:64 + 32 * M + 302 * 2 * M]


def first_diff(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), None)
