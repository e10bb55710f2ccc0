"""numpy model of the dense wire format kosk-dense-v1, written from the format's text alone; it calls nothing
of the library.  Tests only.

Layout: the 24 fields of mpcith_proof in declaration order, each on a 16-byte boundary; Tcomm (4) and comm (23) raw; every u16
field packed two values into three bytes in poly_tobytes bit order (an odd number of stored values gets one trailing zero value);
fields 2, 3, 8, 13, 14, 15, 16 store rows 0..406 only.  Unpack refills rows 407..1303 of those fields by Lagrange interpolation over
GF(3329) through the nodes 256 + rest[j], j < 407, rest the ascending complement of the opened list I."""
import numpy as np

Q = 3329
NPARTY, NOPEN, NCHK, KEPT = 1454, 150, 70, 407
NREST = NPARTY - NOPEN
LISTED = (2, 3, 8, 13, 14, 15, 16)
RAW = (4, 23)
F_I = 5


def field_table(k):
    """[(image offset, image bytes, columns per unopened row or None)] of the 24 fields, from the struct's declaration"""
    eta1 = 3 if k == 2 else 2
    M, E, Z = NCHK + 2 * k + 1, 2 * eta1 + 1, 2 * eta1
    T, R = NOPEN, NREST
    vals = [T * M, T * M, R * NCHK, R * NCHK, None, T, T * k, T * k, R * k, T * k, T * k, T * k, T * k, R * k, R * k, R * k * E, R * k * E,
            T * k * E, T * k * E, T * k * Z, T * k * Z, R * k * Z, R * k * Z, None]
    out, o = [], 0
    for f, v in enumerate(vals):
        size = R * 32 if v is None else 2 * v
        out.append((o, size, v // R if f in LISTED else None))
        o += size
    return out, o


def stored_values(k):
    """per field: number of u16 values the record stores (None for the raw fields)"""
    tab, _ = field_table(k)
    return [None if f in RAW else (KEPT * cols if f in LISTED else size // 2) for f, (_, size, cols) in enumerate(tab)]


def record_layout(k):
    """[(record offset, record bytes)] and the record size"""
    tab, _ = field_table(k)
    out, o = [], 0
    for f, nv in enumerate(stored_values(k)):
        nbytes = tab[f][1] if nv is None else (nv + 1) // 2 * 3
        out.append((o, nbytes))
        o += (nbytes + 15) // 16 * 16
    return out, o


def dense_bytes(k):
    return record_layout(k)[1]


def image_bytes(k):
    return field_table(k)[1]


def pack12(v):
    v = np.asarray(v, dtype=np.uint32)
    if len(v) & 1:
        v = np.concatenate([v, np.zeros(1, np.uint32)])
    a, b = v[0::2], v[1::2]
    out = np.empty((len(a), 3), np.uint8)
    out[:, 0] = a & 0xFF
    out[:, 1] = (a >> 8) | ((b & 0xF) << 4)
    out[:, 2] = b >> 4
    return out.reshape(-1)


def unpack12(raw, n):
    t = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.uint32)
    v = np.empty(2 * len(t), np.uint32)
    v[0::2] = t[:, 0] | ((t[:, 1] & 0xF) << 8)
    v[1::2] = (t[:, 1] >> 4) | (t[:, 2] << 4)
    return v[:n].astype(np.uint16)


_INV = np.array([0] + [pow(a, Q - 2, Q) for a in range(1, Q)], dtype=np.int64)


def lagrange_matrix(opened):
    """L[i - 407][j] of the format's text for a well-formed opened list: the Lagrange basis of the nodes 256 + rest[j], j < 407, at
    the points 256 + rest[i], i = 407..1303 (int64, canonical)"""
    rest = np.array(sorted(set(range(NPARTY)) - set(int(x) for x in opened)), dtype=np.int64)
    assert len(rest) == NREST
    xn, xt = 256 + rest[:KEPT], 256 + rest[KEPT:]
    dn = (xn[:, None] - xn[None, :]) % Q
    np.fill_diagonal(dn, 1)
    den = np.ones(KEPT, np.int64)
    for m in range(KEPT):
        den = den * dn[:, m] % Q
    dt = (xt[:, None] - xn[None, :]) % Q          # never 0: targets are not nodes
    num = np.ones(len(xt), np.int64)
    for m in range(KEPT):
        num = num * dt[:, m] % Q
    # prod_{m != j} (x_i - x_m) / (x_j - x_m) = num_i / (x_i - x_j) / den_j
    return num[:, None] * _INV[dt] % Q * _INV[den][None, :] % Q


def malformed(opened):
    o = [int(x) for x in opened]
    return any(x >= NPARTY for x in o) or len(set(o)) != len(o)


def refill(k, img):
    """rows 407..1303 of the listed fields of a bytearray image from its rows 0..406 and I, in place -> status (1: malformed I, nothing written)"""
    tab, _ = field_table(k)
    opened = np.frombuffer(bytes(img[tab[F_I][0]:tab[F_I][0] + 2 * NOPEN]), np.uint16)
    if malformed(opened):
        return 1
    L = lagrange_matrix(opened)
    for f in LISTED:
        off, size, cols = tab[f]
        rows = np.frombuffer(bytes(img[off:off + size]), np.uint16).reshape(NREST, cols).astype(np.int64)
        fill = (L @ (rows[:KEPT] % Q)) % Q
        img[off + KEPT * cols * 2:off + size] = fill.astype(np.uint16).tobytes()
    return 0


def unpack(k, rec):
    """-> (status, image bytes)"""
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
    """-> (return code, record): 0; -1 a stored value >= 4096; -2 a malformed I or a dropped row that is not the refill"""
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
