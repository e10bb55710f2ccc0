// The registry tree, format kosk-regtree-v1: a Merkle tree over the registry's slots.  Plain C++ and
// KOSK_HD: the sponge states below are what k_registry_tree (kosk_registry.hip) permutes on the GPU, and the functions under them are the
// host definition the C ABI exports (kosk_regtree_*), checked without a GPU by tests/regtree_host_check.cpp.
//   TAG = "kosk-regtree-v1" (15 bytes); every input is one rate-136 block of SHA3-256, the 32-byte operands on 8-byte boundaries
//   leaf of an occupied slot   L(h)   = SHA3-256(TAG || 00 || h[32] || LE32(kyber_k))    52 bytes
//   leaf of an empty slot      E      = SHA3-256(TAG || 01 || LE32(kyber_k))             20 bytes
//   inner node                 N(l,r) = SHA3-256(TAG || 02 || l[32] || r[32])            80 bytes
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "kosk_math.hpp"

namespace kosk {
namespace regtree {

enum { TIER_LEVELS = 10, TIER_INPUTS = 1 << TIER_LEVELS }; // KOSK_REGTREE_TIER_LEVELS: one block reduces 1 024 inputs through 10 levels
constexpr uint64_t TAG0 = 0x6765722d6b736f6bULL; // "kosk-reg"
constexpr uint64_t TAG1 = 0x0031762d65657274ULL; // "tree-v1", the kind byte on top
constexpr uint64_t PAD_END = 0x8000000000000000ULL; // the last bit of the rate block, word 16

KOSK_HD inline void state_head(uint64_t (&s)[25], uint64_t kind)
{
#pragma unroll
    for (int l = 0; l < 25; l++) s[l] = 0;
    s[0] = TAG0;
    s[1] = TAG1 | (kind << 56);
    s[16] = PAD_END;
}
// the absorbed block of L(h): h as four little-endian words
KOSK_HD inline void leaf_state(uint64_t (&s)[25], int K, const uint64_t (&h)[4])
{
    state_head(s, 0);
#pragma unroll
    for (int l = 0; l < 4; l++) s[2 + l] = h[l];
    s[6] = (uint64_t)(uint32_t)K | (0x06ULL << 32);
}
KOSK_HD inline void empty_state(uint64_t (&s)[25], int K)
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

// D: the smallest D with 2^D >= capacity; -1 for capacity < 1
KOSK_HD inline int depth(int capacity)
{
    if (capacity < 1) return -1;
    int d = 0;
    while (((size_t)1 << d) < (size_t)capacity) d++;
    return d;
}
// the tree in HBM, level-major: level l (P >> l nodes of 32 bytes) starts at 32 (2P - (2P >> l)); (2P - 1) 32 bytes in all
KOSK_HD inline size_t level_offset(int D, int l) { return 32 * (((size_t)2 << D) - (((size_t)2 << D) >> l)); }
KOSK_HD inline size_t tree_bytes(int capacity) { return capacity < 1 ? 0 : 32 * (((size_t)2 << depth(capacity)) - 1); }
inline int tiers(int D) { return D <= TIER_LEVELS ? 1 : (D + TIER_LEVELS - 1) / TIER_LEVELS; }
inline int subtrees(int D) { return D <= TIER_LEVELS ? 1 : 1 << (D - TIER_LEVELS); }

// ---- the host definition (any alignment) ----
inline void words_in(uint64_t (&w)[4], const uint8_t *p) { memcpy(w, p, 32); }
inline void digest_out(uint8_t *out, uint64_t (&s)[25])
{
    keccak_f1600(s);
    memcpy(out, s, 32);
}
inline int leaf(int K, const uint8_t *h, uint8_t *out) // h == nullptr: E
{
    if (K < 2 || K > 4 || !out) return -1;
    uint64_t s[25];
    if (h) {
        uint64_t w[4];
        words_in(w, h);
        leaf_state(s, K, w);
    } else {
        empty_state(s, K);
    }
    digest_out(out, s);
    return 0;
}
inline int node(const uint8_t *l, const uint8_t *r, uint8_t *out)
{
    if (!l || !r || !out) return -1;
    uint64_t s[25], a[4], b[4];
    words_in(a, l);
    words_in(b, r);
    node_state(s, a, b);
    digest_out(out, s);
    return 0;
}
// the root that (slot, h or nullptr for "empty", path[depth][32]) implies: step l is N(path[l], cur) where bit l of slot is set, else N(cur, path[l])
inline int root_from_path(int K, int D, int32_t slot, const uint8_t *h, const uint8_t *path, uint8_t *root)
{
    if (K < 2 || K > 4 || D < 0 || D > 31 || slot < 0 || (int64_t)slot >= ((int64_t)1 << D) || !root || (D > 0 && !path)) return -1;
    uint8_t cur[32];
    (void)leaf(K, h, cur);
    for (int l = 0; l < D; l++) {
        const uint8_t *sib = path + (size_t)l * 32;
        if ((slot >> l) & 1) (void)node(sib, cur, cur);
        else (void)node(cur, sib, cur);
    }
    memcpy(root, cur, 32);
    return 0;
}

} // namespace regtree
} // namespace kosk
