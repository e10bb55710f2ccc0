// The registry history, format kosk-reghist-v1: an append-only Merkle tree over the registry's mutation
// events, the shape of RFC 6962.  Plain C++ and KOSK_HD: the sponge states below are what k_reghist_append and k_reghist_frontier
// (kosk_reghist.hip) permute on the GPU, and the functions under them are the host definition the C ABI exports (kosk_reghist_*), checked
// without a GPU by tests/reghist_host_check.cpp.
//   TAG = "kosk-reghist-v1" (15 bytes, the length of the two state trees' tags: the 32-byte operands sit on the same 8-byte boundaries)
//   event leaf       V = SHA3-256(TAG || 00 || h[32] || LE32(op) || LE32(slot) || LE32(kyber_k))                                   60 bytes
//   checkpoint leaf  C = SHA3-256(TAG || 01 || slot_root[32] || sorted_root[32] || LE32(used) || LE32(capacity) || LE32(kyber_k)) 92 bytes
//   inner node       N(l, r) = SHA3-256(TAG || 02 || l[32] || r[32])                                                              80 bytes
//   empty history    O = SHA3-256(TAG || 03 || LE32(kyber_k))                                                                     20 bytes
// The tree over the first n leaves: H(0) = O, H of one leaf is the leaf, and for n > 1 with s the largest power of two below n
// H(D[0:n]) = N(H(D[0:s]), H(D[s:n])).  Node (l, i) is complete at size n iff (i + 1) 2^l <= n and never changes afterwards.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "kosk_regtree.hpp"

namespace kosk {
namespace reghist {

enum { TIER_LEVELS = 10, TIER_INPUTS = 1 << TIER_LEVELS }; // KOSK_REGHIST_TIER_LEVELS: one block owns one aligned group of 1 024 leaves
enum { OP_ADMIT = 1, OP_EVICT = 2, OP_CHECKPOINT = 3 };
enum { EVENT_BYTES = 80, EV_OP = 0, EV_A = 4, EV_B = 8, EV_RESERVED = 12, EV_X = 16, EV_Y = 48 }; // the stored event record
enum { REC_COUNT = 0, REC_INDEX = 4, REC_SIZE = 8, REC_ZERO = 12, REC_NODES = 16 };               // a proof record's header
enum { MAX_EVENTS = 1 << 24, RAGGED_SLOTS = 33 };
constexpr uint64_t TAG0 = regtree::TAG0;         // "kosk-reg"
constexpr uint64_t TAG1 = 0x0031762d74736968ULL; // "hist-v1", the kind byte on top

KOSK_HD inline void state_head(uint64_t (&s)[25], uint64_t kind)
{
#pragma unroll
    for (int l = 0; l < 25; l++) s[l] = 0;
    s[0] = TAG0;
    s[1] = TAG1 | (kind << 56);
    s[16] = regtree::PAD_END;
}
// the absorbed block of V: h as four little-endian words
KOSK_HD inline void event_state(uint64_t (&s)[25], int K, const uint64_t (&h)[4], uint32_t op, uint32_t slot)
{
    state_head(s, 0);
#pragma unroll
    for (int l = 0; l < 4; l++) s[2 + l] = h[l];
    s[6] = (uint64_t)op | ((uint64_t)slot << 32);
    s[7] = (uint64_t)(uint32_t)K | (0x06ULL << 32);
}
KOSK_HD inline void checkpoint_state(uint64_t (&s)[25], int K, const uint64_t (&a)[4], const uint64_t (&b)[4], uint32_t used, uint32_t capacity)
{
    state_head(s, 1);
#pragma unroll
    for (int l = 0; l < 4; l++) { s[2 + l] = a[l]; s[6 + l] = b[l]; }
    s[10] = (uint64_t)used | ((uint64_t)capacity << 32);
    s[11] = (uint64_t)(uint32_t)K | (0x06ULL << 32);
}
KOSK_HD inline void node_state(uint64_t (&s)[25], const uint64_t (&l)[4], const uint64_t (&r)[4])
{
    state_head(s, 2);
#pragma unroll
    for (int i = 0; i < 4; i++) { s[2 + i] = l[i]; s[6 + i] = r[i]; }
    s[10] = 0x06ULL;
}
KOSK_HD inline void empty_state(uint64_t (&s)[25], int K)
{
    state_head(s, 3);
    s[2] = (uint64_t)(uint32_t)K | (0x06ULL << 32);
}

// the smallest d with 2^d >= size; 0 for size 0 or 1; -1 for size < 0
KOSK_HD inline int depth(int size)
{
    if (size < 0) return -1;
    int d = 0;
    while (((size_t)1 << d) < (size_t)size) d++;
    return d;
}
KOSK_HD inline size_t path_bytes(int size) { return size < 1 ? 0 : (size_t)REC_NODES + 32 * (size_t)depth(size); }
KOSK_HD inline size_t consistency_bytes(int size) { return size < 1 ? 0 : (size_t)REC_NODES + 32 * ((size_t)depth(size) + 1); }
// the complete nodes in HBM, level-major over P = 2^depth(max_events) leaf positions (regtree::level_offset)
KOSK_HD inline size_t nodes_bytes(int max_events) { return max_events < 1 ? 0 : 32 * (((size_t)2 << depth(max_events)) - 1); }

// ---- the host definition (any alignment) ----
inline uint32_t le32_in(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline void le32_out(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}
// the leaf of a stored event record: V for ops 1 / 2, C for op 3; -1: bad k, NULL, op outside 1..3, a non-zero reserved field
inline int leaf(int K, const uint8_t *event, uint8_t *out)
{
    if (K < 2 || K > 4 || !event || !out) return -1;
    const uint32_t op = le32_in(event + EV_OP), a = le32_in(event + EV_A), b = le32_in(event + EV_B);
    if (op < OP_ADMIT || op > OP_CHECKPOINT || le32_in(event + EV_RESERVED)) return -1;
    uint64_t s[25], x[4], y[4];
    regtree::words_in(x, event + EV_X);
    regtree::words_in(y, event + EV_Y);
    if (op == OP_CHECKPOINT) {
        checkpoint_state(s, K, x, y, a, b);
    } else {
        if (b || y[0] || y[1] || y[2] || y[3]) return -1;
        event_state(s, K, x, op, a);
    }
    regtree::digest_out(out, s);
    return 0;
}
inline int node(const uint8_t *l, const uint8_t *r, uint8_t *out)
{
    if (!l || !r || !out) return -1;
    uint64_t s[25], a[4], b[4];
    regtree::words_in(a, l);
    regtree::words_in(b, r);
    node_state(s, a, b);
    regtree::digest_out(out, s);
    return 0;
}
inline int empty_root(int K, uint8_t *out)
{
    if (K < 2 || K > 4 || !out) return -1;
    uint64_t s[25];
    empty_state(s, K);
    regtree::digest_out(out, s);
    return 0;
}
// the header agrees with (w1, size), count <= bound, and everything behind the `count` records is zero: count, else -1
inline int record_count(const uint8_t *rec, int w1, int size, int bound)
{
    const uint32_t count = le32_in(rec + REC_COUNT);
    if (le32_in(rec + REC_INDEX) != (uint32_t)w1 || le32_in(rec + REC_SIZE) != (uint32_t)size || le32_in(rec + REC_ZERO) || count > (uint32_t)bound) return -1;
    uint8_t any = 0;
    for (size_t i = (size_t)REC_NODES + 32 * (size_t)count; i < (size_t)REC_NODES + 32 * (size_t)bound; i++) any |= rec[i];
    return any ? -1 : (int)count;
}
// the root that leaf `index` of a history of `size` events and the inclusion record (path_bytes(size) bytes) imply; -1: malformed
inline int root_from_path(int index, int size, const uint8_t *leaf_hash, const uint8_t *rec, uint8_t *root)
{
    if (size < 1 || index < 0 || index >= size || !leaf_hash || !rec || !root) return -1;
    const int count = record_count(rec, index, size, depth(size));
    if (count < 0) return -1;
    uint32_t fn = (uint32_t)index, sn = (uint32_t)size - 1;
    uint8_t r[32];
    memcpy(r, leaf_hash, 32);
    for (int c = 0; c < count; c++) {
        const uint8_t *v = rec + REC_NODES + 32 * (size_t)c;
        if (sn == 0) return -1;
        if ((fn & 1) || fn == sn) {
            (void)node(v, r, r);
            if (!(fn & 1))
                while (fn && !(fn & 1)) { fn >>= 1; sn >>= 1; }
        } else {
            (void)node(r, v, r);
        }
        fn >>= 1; sn >>= 1;
    }
    if (sn != 0) return -1;
    memcpy(root, r, 32);
    return 0;
}
// 1: the history of `size` events under root_new extends the one of old_size events under root_old; 0: the record (consistency_bytes(size)
// bytes) does not show that; -1: bad arguments (a negative size, old_size > size, NULL)
inline int check_consistency(int old_size, int size, const uint8_t *root_old, const uint8_t *root_new, const uint8_t *rec)
{
    if (old_size < 0 || size < 1 || old_size > size || !root_new || !rec || (old_size > 0 && !root_old)) return -1;
    const int count = record_count(rec, old_size, size, depth(size) + 1);
    if (count < 0) return 0;
    if (old_size == 0) return count == 0; // every history extends the empty one: root_old is not read
    if (old_size == size) return count == 0 && !memcmp(root_old, root_new, 32);
    const bool pow2 = !(old_size & (old_size - 1)); // root_old stands in front of the proof
    if (!pow2 && count < 1) return 0;
    uint32_t fn = (uint32_t)old_size - 1, sn = (uint32_t)size - 1;
    while (fn & 1) { fn >>= 1; sn >>= 1; }
    uint8_t fr[32], sr[32];
    memcpy(fr, pow2 ? root_old : rec + REC_NODES, 32);
    memcpy(sr, fr, 32);
    for (int c = pow2 ? 0 : 1; c < count; c++) {
        const uint8_t *v = rec + REC_NODES + 32 * (size_t)c;
        if (sn == 0) return 0;
        if ((fn & 1) || fn == sn) {
            (void)node(v, fr, fr);
            (void)node(v, sr, sr);
            if (!(fn & 1))
                while (fn && !(fn & 1)) { fn >>= 1; sn >>= 1; }
        } else {
            (void)node(sr, v, sr);
        }
        fn >>= 1; sn >>= 1;
    }
    return sn == 0 && !memcmp(fr, root_old, 32) && !memcmp(sr, root_new, 32);
}

} // namespace reghist
} // namespace kosk
