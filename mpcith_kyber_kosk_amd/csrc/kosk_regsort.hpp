// The fingerprint-sorted registry tree, format kosk-regsort-v1: a second Merkle tree over the registry,
// its leaves the occupied slots' (fingerprint, slot) pairs in ascending order, padding behind them.  Two adjacent leaves that straddle a
// fingerprint prove that it is not enrolled.  Plain C++ and KOSK_HD: the sponge states below are what k_regsort_tree (kosk_regsort.hip)
// permutes on the GPU, and the functions under them are the host definition the C ABI exports (kosk_regsort_*), checked without a GPU by
// tests/regsort_host_check.cpp.  The shape (depth, level-major layout, paths, the walk) is that of kosk_regtree.hpp.
//   TAG = "kosk-regsort-v1" (15 bytes, the length of the slot tree's tag: the operands sit on the same 8-byte boundaries)
//   key leaf       S(h, slot) = SHA3-256(TAG || 00 || h[32] || LE32(slot) || LE32(kyber_k))   56 bytes
//   padding leaf   Z          = SHA3-256(TAG || 01 || LE32(kyber_k))                          20 bytes
//   inner node     N(l, r)    = SHA3-256(TAG || 02 || l[32] || r[32])                         80 bytes
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "kosk_regtree.hpp"

namespace kosk {
namespace regsort {

constexpr uint64_t TAG0 = regtree::TAG0;         // "kosk-reg"
constexpr uint64_t TAG1 = 0x0031762d74726f73ULL; // "sort-v1", the kind byte on top

KOSK_HD inline void state_head(uint64_t (&s)[25], uint64_t kind)
{
#pragma unroll
    for (int l = 0; l < 25; l++) s[l] = 0;
    s[0] = TAG0;
    s[1] = TAG1 | (kind << 56);
    s[16] = regtree::PAD_END;
}
// the absorbed block of S(h, slot): h as four little-endian words
KOSK_HD inline void leaf_state(uint64_t (&s)[25], int K, const uint64_t (&h)[4], uint32_t slot)
{
    state_head(s, 0);
#pragma unroll
    for (int l = 0; l < 4; l++) s[2 + l] = h[l];
    s[6] = (uint64_t)slot | ((uint64_t)(uint32_t)K << 32);
    s[7] = 0x06ULL;
}
KOSK_HD inline void pad_state(uint64_t (&s)[25], int K)
{
    state_head(s, 1);
    s[2] = (uint64_t)(uint32_t)K | (0x06ULL << 32);
}
KOSK_HD inline void node_state(uint64_t (&s)[25], const uint64_t (&l)[4], const uint64_t (&r)[4])
{
    state_head(s, 2);
#pragma unroll
    for (int i = 0; i < 4; i++) { s[2 + i] = l[i]; s[6 + i] = r[i]; }
    s[10] = 0x06ULL;
}

// the proof record: 16 bytes of header, h_l, h_r, path_l[D], path_r[D]
enum { REC_POS_L = 0, REC_SLOT_L = 4, REC_SLOT_R = 8, REC_FLAGS = 12, REC_H_L = 16, REC_H_R = 48, REC_PATHS = 80 };
enum { FLAG_LEFT = 1, FLAG_RIGHT = 2, FLAG_RIGHT_KEY = 4, FLAG_PRESENT = 8 };
enum { KIND_NEITHER = 0, KIND_ABSENT = 1, KIND_PRESENT = 2 };
KOSK_HD inline size_t proof_bytes(int D) { return D < 0 || D > 31 ? 0 : (size_t)REC_PATHS + 64 * (size_t)D; }

// ---- the host definition (any alignment) ----
inline int leaf(int K, const uint8_t *h, int32_t slot, uint8_t *out) // h == nullptr: Z
{
    if (K < 2 || K > 4 || !out || (h && slot < 0)) return -1;
    uint64_t s[25];
    if (h) {
        uint64_t w[4];
        regtree::words_in(w, h);
        leaf_state(s, K, w, (uint32_t)slot);
    } else {
        pad_state(s, K);
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
// the root that (pos, h and slot or nullptr for Z, path[depth][32]) implies: step l is N(path[l], cur) where bit l of pos is set, else N(cur, path[l])
inline int root_from_path(int K, int D, int32_t pos, const uint8_t *h, int32_t slot, const uint8_t *path, uint8_t *root)
{
    if (K < 2 || K > 4 || D < 0 || D > 31 || pos < 0 || (int64_t)pos >= ((int64_t)1 << D) || !root || (D > 0 && !path) || (h && slot < 0)) return -1;
    uint8_t cur[32];
    (void)leaf(K, h, slot, cur);
    for (int l = 0; l < D; l++) {
        const uint8_t *sib = path + (size_t)l * 32;
        if ((pos >> l) & 1) (void)node(sib, cur, cur);
        else (void)node(cur, sib, cur);
    }
    memcpy(root, cur, 32);
    return 0;
}
inline int32_t le32_in(const uint8_t *p)
{
    return (int32_t)((uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24);
}
// The decision of check_proof over a record's header and what its operands give: cmp_l = memcmp(h_l, x), cmp_r = memcmp(x, h_r);
// walk_l(): the left walk (pos_l, h_l, slot_l, path_l) gives root; walk_r(): the right walk at pos_l + 1 (S(h_r, slot_r) where bit2 of flags
// is set, else Z) gives root.  Shared by the host function below and k_regsort_check (kosk_relying.hip), which hands in walks it has done
template <class WL, class WR>
KOSK_HD inline int check_decide(int D, int64_t pos_l, uint32_t flags, int cmp_l, int cmp_r, WL &&walk_l, WR &&walk_r)
{
    const int64_t P = (int64_t)1 << D;
    if (flags == (FLAG_LEFT | FLAG_PRESENT))
        return cmp_l == 0 && pos_l >= 0 && pos_l < P && walk_l() ? KIND_PRESENT : KIND_NEITHER;
    const bool left = flags & FLAG_LEFT, right = flags & FLAG_RIGHT, key = flags & FLAG_RIGHT_KEY;
    if ((flags & ~7u) || (!left && !right) || (key && !right)) return KIND_NEITHER;
    if (left) {
        if (pos_l < 0 || pos_l >= P || cmp_l >= 0 || !walk_l()) return KIND_NEITHER;
    } else if (pos_l != -1) {
        return KIND_NEITHER;
    }
    if (right) {
        if (pos_l + 1 >= P) return KIND_NEITHER;
        if (key ? cmp_r >= 0 || !walk_r() : !walk_r()) return KIND_NEITHER;
    } else if (pos_l != P - 1) {
        return KIND_NEITHER;
    }
    return KIND_ABSENT;
}
// what `rec` (proof_bytes(D) bytes) proves about x under `root`: KIND_PRESENT, KIND_ABSENT, KIND_NEITHER; -1 for bad arguments
inline int check_proof(int K, int D, const uint8_t *x, const uint8_t *rec, const uint8_t *root)
{
    if (K < 2 || K > 4 || D < 0 || D > 31 || !x || !rec || !root) return -1;
    const int64_t pos_l = le32_in(rec + REC_POS_L);
    const int32_t slot_l = le32_in(rec + REC_SLOT_L), slot_r = le32_in(rec + REC_SLOT_R);
    const uint32_t flags = (uint32_t)le32_in(rec + REC_FLAGS);
    const uint8_t *h_l = rec + REC_H_L, *h_r = rec + REC_H_R, *path_l = rec + REC_PATHS, *path_r = path_l + (size_t)D * 32;
    uint8_t got[32];
    auto walks = [&](int64_t pos, const uint8_t *h, int32_t slot, const uint8_t *path) {
        return root_from_path(K, D, (int32_t)pos, h, slot, path, got) == 0 && !memcmp(got, root, 32);
    };
    return check_decide(D, pos_l, flags, memcmp(h_l, x, 32), memcmp(x, h_r, 32),
                        [&] { return walks(pos_l, h_l, slot_l, path_l); },
                        [&] { return flags & FLAG_RIGHT_KEY ? walks(pos_l + 1, h_r, slot_r, path_r) : walks(pos_l + 1, nullptr, 0, path_r); });
}

} // namespace regsort
} // namespace kosk
