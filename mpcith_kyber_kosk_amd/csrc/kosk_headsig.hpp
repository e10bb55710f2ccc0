// Signed heads, format kosk-headsig-v1: Winternitz one-time signatures (w = 8, 34 chains of 255 steps)
// under a Merkle tree of 2^h one-time keys, the construction of LMS (RFC 8554) over SHAKE256 with 32-byte outputs.  Plain C++ and KOSK_HD:
// the sponge states below are what the kernels of kosk_headsig.hip permute on the GPU, and the functions under them are the host definition
// the C ABI exports (kosk_headsig_*), checked without a GPU by tests/headsig_host_check.cpp.
//   H(x) = SHAKE256(x, 32 bytes); u32 / u16 / u8 big-endian; I the 16-byte key identifier; q the leaf number, 0 .. 2^h - 1
//   statement   S      = "kosk-sighead-v1" || 00 || root[32] || LE32(size) || LE32(kyber_k)                          56 bytes
//   chain start x_q[i] = H(I || u32(q) || u16(i) || u8(0xFF) || seed)             randomizer C_q: the same with i = 0xFFFD
//   chain step  F      = H(I || u32(q) || u16(i) || u8(j) || t)                    55 bytes: one rate block, t at byte 23
//   one-time pk K_q    = H(I || u32(q) || u16(0x8080) || y_q[0] || ... || y_q[33])  1 110 bytes: nine rate blocks
//   leaf        T[2^h + q] = H(I || u32(2^h + q) || u16(0x8282) || K_q)            inner node T[r] = H(I || u32(r) || u16(0x8383) || T[2r] || T[2r+1])
//   digest      Q      = H(I || u32(q) || u16(0x8181) || C || S)                   110 bytes
// Every operand is carried as little-endian 64-bit words; an operand at byte 22 or 23 of a block is shifted into place (the compiler turns
// the 64-bit shifts into v_alignbit_b32 on the register halves).
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "kosk_kem_dev.hpp"
#include "kosk_regtree.hpp"

namespace kosk {
namespace headsig {

enum { CHAINS = 34, STEPS = 255, MAX_HEIGHT = 24, PUB_BYTES = 52, STATEMENT_BYTES = 56 };
enum { PUB_I = 4, PUB_ROOT = 20, SIG_C = 16, SIG_Z = 48, SIG_PATH = SIG_Z + CHAINS * 32 }; // offsets in the two records
// One block takes ITEMS_PER_BLOCK one-time keys, a lane per (item, chain): 7 x 34 = 238 of 256 lanes
enum { ITEMS_PER_BLOCK = 7, BLOCK_THREADS = 256, Y_WORDS = CHAINS * 4 };
enum { TIER_LEVELS = 10, TIER_INPUTS = 1 << TIER_LEVELS };
enum { LEAF_LAUNCH_MAX = 1 << 16 }; // leaves per launch of k_headsig_leaves: 570 M permutations
enum : uint32_t { TAG_X = 0xFF, TAG_C = 0xFFFD, TAG_K = 0x8080, TAG_Q = 0x8181, TAG_LEAF = 0x8282, TAG_NODE = 0x8383 };
constexpr uint64_t PAD_END = regtree::PAD_END, DOM = 0x1FULL; // SHAKE's domain bits, the last bit of the rate block (word 16)
constexpr uint64_t STMT0 = 0x6769732d6b736f6bULL; // "kosk-sig"
constexpr uint64_t STMT1 = 0x0031762d64616568ULL; // "head-v1", 00

struct Id { uint64_t w[2]; };

KOSK_HD inline uint64_t be32(uint32_t v) { return (uint64_t)((v >> 24) | ((v >> 8) & 0xFF00u) | ((v << 8) & 0xFF0000u) | (v << 24)); }
KOSK_HD inline uint64_t be16(uint32_t v) { return (uint64_t)(((v >> 8) & 0xFFu) | ((v & 0xFFu) << 8)); }
// bytes 16..21 of every hash input: u32(number) || u16(tag or chain)
KOSK_HD inline uint64_t head6(uint32_t number, uint32_t tag) { return be32(number) | be16(tag) << 32; }

KOSK_HD inline void state_clear(uint64_t (&s)[25], const Id &id)
{
#pragma unroll
    for (int l = 0; l < 25; l++) s[l] = 0;
    s[0] = id.w[0];
    s[1] = id.w[1];
    s[16] = PAD_END;
}
// the block of F(q, i, j, t), and with j = 0xFF and t = seed that of x_q[i] (i = 0xFFFD: C_q): t at byte 23
KOSK_HD inline void chain_state(uint64_t (&s)[25], const Id &id, uint64_t head, uint32_t j, const uint64_t (&t)[4])
{
    state_clear(s, id);
    s[2] = head | (uint64_t)j << 48 | t[0] << 56;
    s[3] = t[0] >> 8 | t[1] << 56;
    s[4] = t[1] >> 8 | t[2] << 56;
    s[5] = t[2] >> 8 | t[3] << 56;
    s[6] = t[3] >> 8 | DOM << 56;
}
// I || u32(number) || u16(tag) || NW words, in one rate block (NW <= 11): the operand at byte 22
template <int NW> KOSK_HD inline void tagged_state(uint64_t (&s)[25], const Id &id, uint32_t number, uint32_t tag, const uint64_t (&p)[NW])
{
    static_assert(NW >= 1 && NW <= 11, "one rate block");
    state_clear(s, id);
    s[2] = head6(number, tag) | p[0] << 48;
#pragma unroll
    for (int l = 1; l < NW; l++) s[2 + l] = p[l - 1] >> 16 | p[l] << 48;
    s[2 + NW] = p[NW - 1] >> 16 | DOM << 48;
}
KOSK_HD inline void leaf_state(uint64_t (&s)[25], const Id &id, uint32_t number, const uint64_t (&k)[4]) { tagged_state<4>(s, id, number, TAG_LEAF, k); }
KOSK_HD inline void node_state(uint64_t (&s)[25], const Id &id, uint32_t number, const uint64_t (&l)[4], const uint64_t (&r)[4])
{
    const uint64_t p[8] = {l[0], l[1], l[2], l[3], r[0], r[1], r[2], r[3]};
    tagged_state<8>(s, id, number, TAG_NODE, p);
}
// Q = H(I || u32(q) || u16(0x8181) || C || S), S built from the root's words
KOSK_HD inline void digest_state(uint64_t (&s)[25], const Id &id, uint32_t q, const uint64_t (&c)[4], const uint64_t (&root)[4], uint32_t size, int K)
{
    const uint64_t p[11] = {c[0], c[1], c[2], c[3], STMT0, STMT1, root[0], root[1], root[2], root[3], (uint64_t)size | (uint64_t)(uint32_t)K << 32};
    tagged_state<11>(s, id, q, TAG_Q, p);
}
// a[i]: the bytes of Q, then the checksum's two bytes, high first
KOSK_HD inline uint32_t coefficient(const uint64_t (&Q)[4], int i)
{
    uint32_t cks = 0;
#pragma unroll
    for (int l = 0; l < 4; l++)
#pragma unroll
        for (int b = 0; b < 8; b++) cks += 255u - (uint32_t)((Q[l] >> (8 * b)) & 255u);
    if (i == 32) return cks >> 8;
    if (i == 33) return cks & 255u;
    return (uint32_t)((Q[(i >> 3) & 3] >> (8 * (i & 7))) & 255u);
}
// K_q over nine blocks; Y(l): word l < 136 of y_q[0] || ... || y_q[33].  The state is indexed statically
template <class F> KOSK_HD inline void ots_public_state(uint64_t (&s)[25], const Id &id, uint32_t q, F &&Y)
{
#pragma unroll
    for (int l = 0; l < 25; l++) s[l] = 0;
    const uint64_t h6 = head6(q, TAG_K);
    auto word = [&](int w) -> uint64_t { // word w of the 1 110-byte message, w < 139
        if (w < 2) return w ? id.w[1] : id.w[0]; // no dynamic index: the identifier stays in registers
        const uint64_t lo = w == 2 ? h6 : Y(w - 3) >> 16;
        const uint64_t hi = w - 2 < (int)Y_WORDS ? Y(w - 2) << 48 : DOM << 48;
        return lo | hi;
    };
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int blk = 0; blk < 8; blk++) {
#pragma unroll
        for (int l = 0; l < 17; l++) s[l] ^= word(17 * blk + l);
        kem::perm(s);
    }
    s[0] ^= word(136);
    s[1] ^= word(137);
    s[2] ^= word(138);
    s[16] ^= PAD_END;
}

KOSK_HD inline size_t sig_bytes(int h) { return h < 1 || h > MAX_HEIGHT ? 0 : (size_t)SIG_PATH + 32 * (size_t)h; }
// the tree in HBM, heap order: T[r] at 32 r, r = 1 .. 2^(h+1) - 1 (slot 0 is unused)
KOSK_HD inline size_t tree_bytes(int h) { return (size_t)64 << h; }

// ---- the host definition (any alignment) ----
inline uint32_t le32_in(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
inline void le32_out(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t)v; p[1] = (uint8_t)(v >> 8); p[2] = (uint8_t)(v >> 16); p[3] = (uint8_t)(v >> 24);
}
inline void wipe_words(uint64_t *p, int n) // not removed as a dead store
{
    volatile uint64_t *v = p;
    for (int l = 0; l < n; l++) v[l] = 0;
}
inline void id_in(Id &id, const uint8_t *p) { memcpy(id.w, p, 16); }
inline void finish(uint64_t (&s)[25], uint64_t (&out)[4])
{
    kem::perm(s);
    for (int l = 0; l < 4; l++) out[l] = s[l];
}
inline int statement(int K, const uint8_t *root, int size, uint8_t *out)
{
    if (K < 2 || K > 4 || !root || size < 0 || !out) return -1;
    memcpy(out, &STMT0, 8);
    memcpy(out + 8, &STMT1, 8);
    memmove(out + 16, root, 32);
    le32_out(out + 48, (uint32_t)size);
    le32_out(out + 52, (uint32_t)K);
    return 0;
}
// x_q[i] (i < 34) or C_q (i = TAG_C)
inline void secret_start(const Id &id, uint32_t q, uint32_t i, const uint64_t (&seed)[4], uint64_t (&out)[4])
{
    uint64_t s[25];
    chain_state(s, id, head6(q, i), TAG_X, seed);
    finish(s, out);
}
inline void chain_run(const Id &id, uint32_t q, uint32_t i, int from, int to, uint64_t (&t)[4])
{
    uint64_t s[25];
    for (int j = from; j < to; j++) {
        chain_state(s, id, head6(q, i), (uint32_t)j, t);
        finish(s, t);
    }
}
// T[2^h + q] from the 34 chain ends
inline void leaf_from_ends(const Id &id, int h, uint32_t q, const uint64_t (&y)[Y_WORDS], uint64_t (&out)[4])
{
    uint64_t s[25], k[4];
    ots_public_state(s, id, q, [&](int l) { return y[l]; });
    finish(s, k);
    leaf_state(s, id, ((uint32_t)1 << h) + q, k);
    finish(s, out);
}
// 1 / 0 / -1 (NULL, bad k, size < 0, a height outside 1..24 in pub)
inline int verify(const uint8_t *pub, int K, const uint8_t *root, int size, const uint8_t *sig)
{
    if (!pub || K < 2 || K > 4 || !root || size < 0 || !sig) return -1;
    const uint32_t h = le32_in(pub);
    if (h < 1 || h > MAX_HEIGHT) return -1;
    if (le32_in(sig) != h || le32_in(sig + 4) != (uint32_t)size || ((uint32_t)size >> h) != 0 || le32_in(sig + 8) || le32_in(sig + 12)) return 0;
    const uint32_t q = (uint32_t)size;
    Id id;
    id_in(id, pub + PUB_I);
    uint64_t s[25], c[4], r[4], Q[4], y[Y_WORDS], cur[4];
    memcpy(c, sig + SIG_C, 32);
    memcpy(r, root, 32);
    digest_state(s, id, q, c, r, (uint32_t)size, K);
    finish(s, Q);
    for (int i = 0; i < CHAINS; i++) {
        uint64_t t[4];
        memcpy(t, sig + SIG_Z + 32 * i, 32);
        chain_run(id, q, (uint32_t)i, (int)coefficient(Q, i), STEPS, t);
        memcpy(y + 4 * i, t, 32);
    }
    leaf_from_ends(id, (int)h, q, y, cur);
    uint32_t number = ((uint32_t)1 << h) + q;
    for (uint32_t l = 0; l < h; l++) {
        uint64_t sib[4];
        memcpy(sib, sig + SIG_PATH + 32 * l, 32);
        if (number & 1) node_state(s, id, number >> 1, sib, cur);
        else node_state(s, id, number >> 1, cur, sib);
        finish(s, cur);
        number >>= 1;
    }
    return memcmp(cur, pub + PUB_ROOT, 32) == 0;
}
// the public key of (height, seed, id) on one thread: 2^h x (34 x 256 + 10) + 2^h - 1 permutations, a stack of h + 1 nodes
inline int public_from_seed(int h, const uint8_t *seed, const uint8_t *idp, uint8_t *pub)
{
    if (h < 1 || h > MAX_HEIGHT || !seed || !idp || !pub) return -1;
    Id id;
    id_in(id, idp);
    uint64_t sd[4], stack[MAX_HEIGHT + 1][4], y[Y_WORDS], s[25];
    memcpy(sd, seed, 32);
    for (uint32_t q = 0; !(q >> h); q++) {
        for (int i = 0; i < CHAINS; i++) {
            uint64_t t[4];
            secret_start(id, q, (uint32_t)i, sd, t);
            chain_run(id, q, (uint32_t)i, 0, STEPS, t);
            memcpy(y + 4 * i, t, 32);
        }
        uint64_t cur[4];
        leaf_from_ends(id, h, q, y, cur);
        uint32_t number = ((uint32_t)1 << h) + q;
        int l = 0;
        for (; (number & 1) && number > 1; l++, number >>= 1) { // a right child: its left sibling waits on the stack
            node_state(s, id, number >> 1, stack[l], cur);
            finish(s, cur);
        }
        memcpy(stack[l], cur, 32);
    }
    wipe_words(sd, 4);
    wipe_words(y, Y_WORDS);
    le32_out(pub, (uint32_t)h);
    memmove(pub + PUB_I, idp, 16);
    memcpy(pub + PUB_ROOT, stack[h], 32);
    return 0;
}

} // namespace headsig
} // namespace kosk
