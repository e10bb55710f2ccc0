"""numpy model of the dense wire format kosk-dense-v2, written from the format's text alone; it calls nothing of the
library.  Tests only.  The byte layout rule is v1's (the helpers of tests/dense_model.py); what differs is the number of stored rows:

  fields 2, 3, 8, 13, 14   rows 0..406, refilled as in v1 (plain Lagrange interpolation through the first 407 nodes);
  fields 15, 16            rows 0..150; column c shares kappa_c = (c mod (2 eta1 + 1)) - eta1 mod q at the 256 packed positions;
  fields 21, 22            rows 0..556; zero at the 256 packed positions (kappa = 0).

For R stored rows, x_j = 256 + rest[j], Z(x) = prod_{a < 256} (x - a), every row i >= R is
  v_j = (y[j][c] mod q - kappa_c) / Z(x_j),  out[i][c] = kappa_c + Z(x_i) sum_{j < R} v_j prod_{m < R, m != j} (x_i - x_m) / (x_j - x_m)."""
import numpy as np

from tests.dense_model import (F_I, NCHK, NOPEN, NPARTY, NREST, Q, RAW, field_table as _v1_field_table, image_bytes, malformed,  # noqa: F401
                               pack12, unpack12)

ROWS = {2: 407, 3: 407, 8: 407, 13: 407, 14: 407, 15: 151, 16: 151, 21: 557, 22: 557}   # field -> stored rows
LISTED = tuple(sorted(ROWS))
ETA_FIELDS, U_FIELDS = (15, 16), (21, 22)

_INV = np.array([0] + [pow(a, Q - 2, Q) for a in range(1, Q)], dtype=np.int64)


def eta1(k):
    return 3 if k == 2 else 2


def field_table(k):
    """[(image offset, image bytes, columns per unopened row or None)]: v1's table, with the columns of fields 21, 22 as well"""
    tab, total = _v1_field_table(k)
    tab = list(tab)
    for f in U_FIELDS:
        off, size, _ = tab[f]
        tab[f] = (off, size, size // 2 // NREST)
    return tab, total


def stored_values(k):
    tab, _ = field_table(k)
    return [None if f in RAW else (ROWS[f] * cols if f in ROWS else size // 2) for f, (_, size, cols) in enumerate(tab)]


def record_layout(k):
    """[(record offset, record bytes)] and the record size: every field on a 16-byte boundary, 12 bits per stored value, an odd count
    with one trailing zero value"""
    tab, _ = field_table(k)
    out, o = [], 0
    for f, nv in enumerate(stored_values(k)):
        nbytes = tab[f][1] if nv is None else (nv + 1) // 2 * 3
        out.append((o, nbytes))
        o += (nbytes + 15) // 16 * 16
    return out, o


def dense2_bytes(k):
    return record_layout(k)[1]


def kappa(k, f, cols):
    """the public constant of every column of field f"""
    if f in ETA_FIELDS:
        e = eta1(k)
        return (np.arange(cols, dtype=np.int64) % (2 * e + 1) - e) % Q
    return np.zeros(cols, np.int64)


def rest_of(opened):
    rest = np.array(sorted(set(range(NPARTY)) - set(int(x) for x in opened)), dtype=np.int64)
    assert len(rest) == NREST
    return rest


def zeta(x):
    """Z(x) = prod_{a < 256} (x - a) mod q for an array of points"""
    z = np.ones(len(x), np.int64)
    for a in range(256):
        z = z * ((x - a) % Q) % Q
    return z


def lagrange_matrix(rest, R):
    """L[i - R][j] = prod_{m < R, m != j} (x_i - x_m) / (x_j - x_m), i = R..1303, j < R"""
    xn, xt = 256 + rest[:R], 256 + rest[R:]
    dn = (xn[:, None] - xn[None, :]) % Q
    np.fill_diagonal(dn, 1)
    den = np.ones(R, np.int64)
    for m in range(R):
        den = den * dn[:, m] % Q
    dt = (xt[:, None] - xn[None, :]) % Q          # never 0: targets are not nodes
    num = np.ones(len(xt), np.int64)
    for m in range(R):
        num = num * dt[:, m] % Q
    return num[:, None] * _INV[dt] % Q * _INV[den][None, :] % Q


def refill_field(k, f, rest, kept, mats=None):
    """the dropped rows [1304 - R][cols] of field f from its kept rows [R][cols] (any u16)"""
    R = ROWS[f]
    L = mats[R] if mats is not None else lagrange_matrix(rest, R)
    y = np.asarray(kept, np.int64) % Q
    if R == 407:
        return (L @ y) % Q
    kap = kappa(k, f, y.shape[1])
    x = 256 + rest
    z = zeta(x)
    v = (y - kap[None, :]) % Q * _INV[z[:R]][:, None] % Q
    return (kap[None, :] + z[R:, None] * ((L @ v) % Q)) % Q


def refill(k, img):
    """the dropped rows of the nine fields of a bytearray image from its kept rows and I, in place -> status (1: malformed I, nothing written)"""
    tab, _ = field_table(k)
    opened = np.frombuffer(bytes(img[tab[F_I][0]:tab[F_I][0] + 2 * NOPEN]), np.uint16)
    if malformed(opened):
        return 1
    rest = rest_of(opened)
    mats = {R: lagrange_matrix(rest, R) for R in sorted(set(ROWS.values()))}
    for f in LISTED:
        off, size, cols = tab[f]
        R = ROWS[f]
        rows = np.frombuffer(bytes(img[off:off + R * cols * 2]), np.uint16).reshape(R, cols)
        img[off + R * cols * 2:off + size] = refill_field(k, f, rest, rows, mats).astype(np.uint16).tobytes()
    return 0


def unpack(k, rec):
    """-> (status, image bytes); status 1: a malformed I, all dropped rows zero"""
    tab, total = field_table(k)
    lay, size = record_layout(k)
    assert len(rec) == size
    img = bytearray(total)
    for f, nv in enumerate(stored_values(k)):
        ro, rb = lay[f]
        if nv is None:
            img[tab[f][0]:tab[f][0] + tab[f][1]] = rec[ro:ro + rb]
        else:
            img[tab[f][0]:tab[f][0] + 2 * nv] = unpack12(rec[ro:ro + rb], nv).tobytes()
    status = refill(k, img)
    return status, bytes(img)


def pack(k, img):
    """-> (return code, record): 0; -1 a stored value >= 4096 (it wins); -2 a malformed I or a dropped u16 that is not the refill"""
    tab, total = field_table(k)
    lay, size = record_layout(k)
    assert len(img) == total
    rec = bytearray(size)
    for f, nv in enumerate(stored_values(k)):
        ro, rb = lay[f]
        if nv is None:
            rec[ro:ro + rb] = img[tab[f][0]:tab[f][0] + tab[f][1]]
            continue
        v = np.frombuffer(bytes(img[tab[f][0]:tab[f][0] + 2 * nv]), np.uint16)
        if (v >= 4096).any():
            return -1, None
        rec[ro:ro + rb] = pack12(v).tobytes()
    status, back = unpack(k, bytes(rec))
    if status or back != bytes(img):
        return -2, None
    return 0, bytes(rec)
