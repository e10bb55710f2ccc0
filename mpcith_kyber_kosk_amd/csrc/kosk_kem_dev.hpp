// Device functions of the Kyber KEM (kyber/kem.c:76-96, :140-169; indcpa_enc / indcpa_dec, kyber/indcpa.c:264-336) for
// kosk_kem_kernels.hip.  Everything here is KOSK_HD and written per work item (`tid` of `nthr` cooperating threads, barriers
// through KEM_SYNC): a host build runs a whole block as tid 0 of 1, which is how tools/kem_host_model.cpp checks these very
// functions against the fixture without a GPU.
//
// Arithmetic: canonical residues in [0, q) throughout.  ct and ss depend only on residues, so the reference's Montgomery
// bookkeeping is not followed: the zetas are the plain 17^bitrev7(k), basemul is the plain product in Z_q[X]/(X^2 - zeta), and the
// inverse NTT ends with one multiplication by 128^-1.
//
// Secrets (decapsulation): no branch and no address below depends on s, m', the comparison result or z.  The conditional
// subtractions are arithmetic (sign mask), compression is the integer expression, the comparison is an OR over byte differences and
// the select is a mask.  Only gen_matrix's rejection sampling (public: rho) branches on data.
#pragma once
#include "kosk_math.hpp"
#if defined(__HIPCC__)
#include "kosk_keccak_dev.hpp"
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define KEM_SYNC() __syncthreads()
#else
#define KEM_SYNC() ((void)0)
#endif

namespace kosk {
namespace kem {

struct alignas(16) U128 { uint32_t x, y, z, w; };

// sizes of one parameter set (kyber/params.h)
struct Dims {
    int K, eta1, du, dv;
    int pvb;       // KYBER_POLYVECBYTES = 384 K
    int pk, sk;    // 384 K + 32, 768 K + 96
    int ub, ct;    // compressed u: 32 K du; ciphertext: ub + 32 dv
};
KOSK_HD inline Dims dims(int K)
{
    Dims d;
    d.K = K;
    d.eta1 = K == 2 ? 3 : 2;
    d.du = K == 4 ? 11 : 10;
    d.dv = K == 4 ? 5 : 4;
    d.pvb = 384 * K;
    d.pk = d.pvb + 32;
    d.sk = 2 * d.pvb + 96;
    d.ub = 32 * K * d.du;
    d.ct = d.ub + 32 * d.dv;
    return d;
}

// ------------------------------------------------------------------------------------------------------------ field --
KOSK_HD inline uint32_t csub(uint32_t x) // x in [0, 2q) -> [0, q), no branch
{
    const uint32_t t = x - (uint32_t)Q;
    return t + ((uint32_t)((int32_t)t >> 31) & (uint32_t)Q);
}
KOSK_HD inline uint32_t mulq(uint32_t a, uint32_t b) { return a * b % (uint32_t)Q; } // a, b < 2^16
// ⌊(x 2^d + ⌊q/2⌋) / q⌋ mod 2^d for x in [0, q): the integer expression itself (poly.c:33, :53, polyvec.c:27, :57; poly.c:202)
KOSK_HD inline uint32_t compress(uint32_t x, int d) { return (((x << d) + (uint32_t)(Q / 2)) / (uint32_t)Q) & ((1u << d) - 1u); }
// poly.c:98-122, polyvec.c:95-141: (t q + 2^(d-1)) >> d
KOSK_HD inline uint32_t decompress(uint32_t t, int d) { return (t * (uint32_t)Q + (1u << (d - 1))) >> d; }

// plain zetas 17^bitrev7(k) mod q in [0, q) (ntt.c:39-56 holds them times 2^16)
struct ZetaPlain {
    uint16_t z[128];
    constexpr ZetaPlain() : z()
    {
        int32_t pw[128] = {};
        pw[0] = 1;
        for (int i = 1; i < 128; i++) pw[i] = pw[i - 1] * 17 % Q;
        for (int i = 0; i < 128; i++) {
            int br = 0;
            for (int b = 0; b < 7; b++) br |= ((i >> b) & 1) << (6 - b);
            z[i] = (uint16_t)pw[br];
        }
    }
};
static constexpr ZetaPlain kZetaPlain{};
#if defined(__HIPCC__)
__constant__ static const ZetaPlain kZetaPlainDev{};
#endif
KOSK_HD inline uint32_t zeta(int k)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return kZetaPlainDev.z[k];
#else
    return kZetaPlain.z[k];
#endif
}
constexpr uint32_t INV128 = 3303; // 128 * 3303 = 127 q + 1

// ------------------------------------------------------------------------------------------- NTT on a tile in LDS --
// `np` polynomials of 256 u16 in [0, q), back to back at `L`; every layer is np x 128 independent butterflies dealt to the threads
// of the workgroup, one barrier per layer (ntt.c:80-95)
KOSK_HD inline void ntt_tile(uint16_t *L, int np, int tid, int nthr)
{
    for (int len = 128; len >= 2; len >>= 1) {
        for (int w = tid; w < np * 128; w += nthr) {
            const int p = w >> 7, b = w & 127, grp = b / len, j = grp * 2 * len + (b - grp * len);
            uint16_t *r = L + p * 256;
            const uint32_t t = mulq(zeta(128 / len + grp), r[j + len]), a = r[j];
            r[j + len] = (uint16_t)csub(a + (uint32_t)Q - t);
            r[j] = (uint16_t)csub(a + t);
        }
        KEM_SYNC();
    }
}
// the mirror (ntt.c:106-126: Gentleman-Sande layers with zetas[127 - ...]); the final factor 128^-1 is left to the consumer (INV128)
KOSK_HD inline void invntt_tile(uint16_t *L, int np, int tid, int nthr)
{
    for (int len = 2; len <= 128; len <<= 1) {
        for (int w = tid; w < np * 128; w += nthr) {
            const int p = w >> 7, b = w & 127, grp = b / len, j = grp * 2 * len + (b - grp * len);
            uint16_t *r = L + p * 256;
            const uint32_t a = r[j], c = r[j + len];
            r[j] = (uint16_t)csub(a + c);
            r[j + len] = (uint16_t)mulq(zeta(2 * (128 / len) - 1 - grp), c + (uint32_t)Q - a);
        }
        KEM_SYNC();
    }
}

// eight 12-bit values from 12 bytes at a 4-byte aligned address (poly_frombytes, poly.c:150-158), folded mod q as the reference's
// arithmetic does with them
KOSK_HD inline void unpack12x8(const uint8_t *p, uint32_t (&c)[8]) // the fields as they stand, in [0, 4096)
{
    const uint32_t *w = reinterpret_cast<const uint32_t *>(p);
    const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
    c[0] = w0 & 0xFFF; c[1] = (w0 >> 12) & 0xFFF; c[2] = ((w0 >> 24) | (w1 << 8)) & 0xFFF; c[3] = (w1 >> 4) & 0xFFF;
    c[4] = (w1 >> 16) & 0xFFF; c[5] = ((w1 >> 28) | (w2 << 4)) & 0xFFF; c[6] = (w2 >> 8) & 0xFFF; c[7] = w2 >> 20;
}
KOSK_HD inline void load12x8(const uint8_t *p, uint32_t (&c)[8])
{
    unpack12x8(p, c);
#pragma unroll
    for (int i = 0; i < 8; i++) c[i] = csub(c[i]);
}
// the inverse for eight canonical residues (poly_tobytes, poly.c:128-147): 12 bytes at a 4-byte aligned address
KOSK_HD inline void store12x8(uint8_t *p, const uint32_t (&c)[8])
{
    uint32_t *w = reinterpret_cast<uint32_t *>(p);
    w[0] = c[0] | (c[1] << 12) | (c[2] << 24);
    w[1] = (c[2] >> 8) | (c[3] << 4) | (c[4] << 16) | (c[5] << 28);
    w[2] = (c[5] >> 4) | (c[6] << 8) | (c[7] << 20);
}
KOSK_HD inline void load16x8(const void *p, uint32_t (&c)[8]) // eight u16 at a 16-byte aligned address: one 16-byte load
{
    const U128 v = *reinterpret_cast<const U128 *>(p);
    c[0] = v.x & 0xFFFF; c[1] = v.x >> 16; c[2] = v.y & 0xFFFF; c[3] = v.y >> 16;
    c[4] = v.z & 0xFFFF; c[5] = v.z >> 16; c[6] = v.w & 0xFFFF; c[7] = v.w >> 16;
}
KOSK_HD inline void store16x8(void *p, const uint32_t (&c)[8])
{
    U128 v;
    v.x = c[0] | (c[1] << 16); v.y = c[2] | (c[3] << 16); v.z = c[4] | (c[5] << 16); v.w = c[6] | (c[7] << 16);
    *reinterpret_cast<U128 *>(p) = v;
}
// acc += a * b in Z_q[X]/(X^2 - zeta) for the four coefficient pairs of group g (coefficients 8 g .. 8 g + 7): pairs 0, 1 belong
// to zeta[64 + 2 g] (+, -), pairs 2, 3 to zeta[64 + 2 g + 1] (ntt.c:139-146, poly.c:290-297)
KOSK_HD inline void basemul8_acc(uint32_t (&acc)[8], const uint32_t (&a)[8], const uint32_t (&b)[8], int g)
{
#pragma unroll
    for (int p = 0; p < 4; p++) {
        const uint32_t z = zeta(64 + 2 * g + (p >> 1));
        uint32_t t = mulq(mulq(a[2 * p + 1], b[2 * p + 1]), z);
        if (p & 1) t = (uint32_t)Q - t; // in (0, q]
        acc[2 * p] = (acc[2 * p] + mulq(a[2 * p], b[2 * p]) + t) % (uint32_t)Q;
        acc[2 * p + 1] = (acc[2 * p + 1] + a[2 * p] * b[2 * p + 1] + a[2 * p + 1] * b[2 * p]) % (uint32_t)Q;
    }
}

// ---------------------------------------------------------------------------------------------------------- Keccak --
KOSK_HD inline void perm(uint64_t (&s)[25])
{
#if defined(__HIP_DEVICE_COMPILE__)
    KState k;
#pragma unroll
    for (int l = 0; l < 25; l++) { k.lo[l] = (uint32_t)s[l]; k.hi[l] = (uint32_t)(s[l] >> 32); }
    keccak_f1600_dev(k);
#pragma unroll
    for (int l = 0; l < 25; l++) s[l] = (uint64_t)k.lo[l] | ((uint64_t)k.hi[l] << 32);
#else
    keccak_f1600(s);
#endif
}
KOSK_HD inline void zero(uint64_t (&s)[25])
{
#pragma unroll
    for (int l = 0; l < 25; l++) s[l] = 0;
}
// rate-136 sponge (sha3_256: dom 0x06, shake256: dom 0x1F) over a message of `nwords` 64-bit words fetched by index; the state is
// only ever indexed statically
template <class F>
KOSK_HD inline void absorb136(uint64_t (&s)[25], F fetch, int nwords, uint64_t dom)
{
    zero(s);
    int done = 0;
    while (nwords - done >= 17) {
#pragma unroll
        for (int l = 0; l < 17; l++) s[l] ^= fetch(done + l);
        perm(s);
        done += 17;
    }
    const int rem = nwords - done;
#pragma unroll
    for (int l = 0; l < 17; l++) {
        if (l < rem) s[l] ^= fetch(done + l);
        if (l == rem) s[l] ^= dom;
    }
    s[16] ^= 0x8000000000000000ULL;
    perm(s);
}
// hash_g (sha3_512) of m[32] || h[32]: kr = K-bar || coins (kem.c:88-89, :154-155)
KOSK_HD inline void hash_g64(const uint64_t (&m)[4], const uint64_t (&h)[4], uint64_t (&kr)[8])
{
    uint64_t s[25];
    zero(s);
#pragma unroll
    for (int l = 0; l < 4; l++) { s[l] = m[l]; s[4 + l] = h[l]; }
    s[8] = 0x06ULL ^ 0x8000000000000000ULL; // rate 72: pad start and end share word 8
    perm(s);
#pragma unroll
    for (int l = 0; l < 8; l++) kr[l] = s[l];
}

// 16 cbd2 coefficients of one 64-bit word / 4 cbd3 coefficients of 24 bits (cbd.c:58-107), as int16 pairs
KOSK_HD inline void cbd2_word(uint64_t x, int16_t *out) // out 16-byte aligned, 32 bytes
{
    const uint64_t d = (x & 0x5555555555555555ULL) + ((x >> 1) & 0x5555555555555555ULL);
    uint32_t c[16];
#pragma unroll
    for (int j = 0; j < 16; j++) c[j] = (uint32_t)((int32_t)((d >> (4 * j)) & 3) - (int32_t)((d >> (4 * j + 2)) & 3)) & 0xFFFFu;
    uint32_t lo[8], hi[8];
#pragma unroll
    for (int j = 0; j < 8; j++) { lo[j] = c[j]; hi[j] = c[8 + j]; }
    store16x8(out, lo);
    store16x8(out + 8, hi);
}
KOSK_HD inline uint64_t cbd3_triple(uint32_t x)
{
    const uint32_t d = (x & 0x00249249u) + ((x >> 1) & 0x00249249u) + ((x >> 2) & 0x00249249u);
    uint64_t r = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t c = (uint32_t)((int32_t)((d >> (6 * j)) & 7) - (int32_t)((d >> (6 * j + 3)) & 7)) & 0xFFFFu;
        r |= (uint64_t)c << (16 * j);
    }
    return r;
}
// the 24 bits at bit offset 24 T of a byte string held as 64-bit words (static word indices after unrolling)
template <int NW>
KOSK_HD inline uint32_t triple_at(const uint64_t (&w)[NW], int T)
{
    const int bit = 24 * T, k = bit >> 6, sh = bit & 63;
    uint64_t x = w[k] >> sh;
    if (sh > 40) x |= w[k + 1 < NW ? k + 1 : k] << (64 - sh);
    return (uint32_t)x & 0xFFFFFFu;
}

// poly_getnoise_eta{1,2}: prf = SHAKE256(coins[32] || nonce) (symmetric-shake.c), 64 eta bytes, cbd_eta (poly.c:225-247); small
// signed coefficients as int16
KOSK_HD inline void noise_poly(const uint64_t (&coins)[4], int nonce, int eta, int16_t *out)
{
    uint64_t s[25];
    zero(s);
#pragma unroll
    for (int l = 0; l < 4; l++) s[l] = coins[l];
    s[4] = (uint64_t)(uint32_t)nonce | (0x1FULL << 8);
    s[16] = 0x8000000000000000ULL;
    perm(s);
    if (eta == 2) {
#pragma unroll
        for (int l = 0; l < 16; l++) cbd2_word(s[l], out + 16 * l);
        return;
    }
    uint64_t w[24];
#pragma unroll
    for (int l = 0; l < 17; l++) w[l] = s[l];
    perm(s);
#pragma unroll
    for (int l = 0; l < 7; l++) w[17 + l] = s[l];
#pragma unroll
    for (int T = 0; T < 64; T++) reinterpret_cast<uint64_t *>(out)[T] = cbd3_triple(triple_at<24>(w, T));
}

// one entry of gen_matrix (indcpa.c:168-193): SHAKE128(rho || x || y), rej_uniform until 256 coefficients.  Public data: the
// loop and the stores branch on it.  Returns false when `max_blocks` blocks did not suffice (the reference would squeeze on).
KOSK_HD inline bool matrix_entry(const uint64_t (&rho)[4], int x, int y, int max_blocks, int16_t *out)
{
    uint64_t s[25];
    zero(s);
#pragma unroll
    for (int l = 0; l < 4; l++) s[l] = rho[l];
    s[4] = (uint64_t)(uint32_t)x | ((uint64_t)(uint32_t)y << 8) | (0x1FULL << 16);
    s[20] = 0x8000000000000000ULL; // rate 168
    int ctr = 0, blocks = 0;
    while (ctr < 256) {
        if (blocks == max_blocks) return false;
        perm(s);
        blocks++;
        uint64_t w[21];
#pragma unroll
        for (int l = 0; l < 21; l++) w[l] = s[l];
#pragma unroll
        for (int T = 0; T < 56; T++) {
            const uint32_t t = triple_at<21>(w, T), d1 = t & 0xFFF, d2 = t >> 12;
            if (d1 < (uint32_t)Q && ctr < 256) out[ctr++] = (int16_t)d1;
            if (d2 < (uint32_t)Q && ctr < 256) out[ctr++] = (int16_t)d2;
        }
    }
    return true;
}

KOSK_HD inline uint64_t ld64(const uint8_t *p, int i) { return reinterpret_cast<const uint64_t *>(p)[i]; }

// ------------------------------------------------------------------------------------------------- the hash roles --
// sha3_256 of `nbytes` (a multiple of 8) at the 8-byte aligned p
KOSK_HD inline void sha3_256_words(const uint8_t *p, int nbytes, uint64_t (&h)[4])
{
    uint64_t s[25];
    absorb136(s, [&](int i) { return ld64(p, i); }, nbytes / 8, 0x06ULL);
#pragma unroll
    for (int l = 0; l < 4; l++) h[l] = s[l];
}
// rkprf = SHAKE256(z[32] || ct) (symmetric-shake.c: kyber_shake256_rkprf); both 8-byte aligned.  z is secret: it is data only.
KOSK_HD inline void rkprf(const uint8_t *z, const uint8_t *ct, int ct_bytes, uint64_t (&out)[4])
{
    uint64_t s[25];
    absorb136(s, [&](int i) { return i < 4 ? ld64(z, i) : ld64(ct, i - 4); }, 4 + ct_bytes / 8, 0x1FULL);
#pragma unroll
    for (int l = 0; l < 4; l++) out[l] = s[l];
}

// --------------------------------------------------------------------------------------------------- indcpa_enc --
// One workgroup, one item.  LDS tile L: (2 K + 1) polynomials of 256 u16 -- r-hat[K] | u[K] | v.
//   pk    : 384 K bytes of t-hat (12-bit, any value: folded mod q)           A : A^T[K][K][256] int16 in [0, q), 16-byte aligned
//   noise : r[K] | e1[K] | e2, int16[256] each, 16-byte aligned               m : the 32 message bytes
// The ciphertext bytes go to ct_out, or (ct_out == nullptr) are compared with ct_cmp: the return value is the OR of this thread's
// byte differences.
KOSK_HD inline uint32_t encrypt_block(const Dims &D, uint16_t *L, int tid, int nthr, const uint8_t *pk, const int16_t *A, const int16_t *noise,
                                      const uint8_t *m, uint8_t *ct_out, const uint8_t *ct_cmp)
{
    const int K = D.K;
    uint16_t *R = L, *O = L + K * 256;
    // r as residues
    for (int w = tid; w < K * 32; w += nthr) {
        uint32_t c[8];
        load16x8(noise + 8 * w, c);
#pragma unroll
        for (int i = 0; i < 8; i++) { const int32_t e = (int16_t)c[i]; c[i] = (uint32_t)(e + ((e >> 31) & Q)); }
        store16x8(R + 8 * w, c);
    }
    KEM_SYNC();
    ntt_tile(R, K, tid, nthr);
    // u-hat_o = sum_j A^T[o][j] o r-hat_j (o < K),  v-hat = sum_j t-hat_j o r-hat_j (o == K)
    for (int w = tid; w < (K + 1) * 32; w += nthr) {
        const int o = w >> 5, g = w & 31;
        uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int j = 0; j < K; j++) {
            uint32_t a[8], b[8];
            if (o < K) load16x8(A + ((o * K + j) * 256 + 8 * g), a);
            else load12x8(pk + j * 384 + 12 * g, a);
            load16x8(R + j * 256 + 8 * g, b);
            basemul8_acc(acc, a, b, g);
        }
        store16x8(O + o * 256 + 8 * g, acc);
    }
    KEM_SYNC();
    invntt_tile(O, K + 1, tid, nthr);
    // + e1 / + e2 + frommsg(m), compress, pack: eight coefficients are d bytes of a little-endian bit stream (polyvec.c:17-86, poly.c:19-81)
    uint32_t diff = 0;
    for (int w = tid; w < (K + 1) * 32; w += nthr) {
        const int o = w >> 5, g = w & 31, d = o < K ? D.du : D.dv;
        const int at = o < K ? (o * 32 + g) * D.du : D.ub + g * D.dv;
        uint32_t x[8], e[8];
        load16x8(O + o * 256 + 8 * g, x);
        load16x8(noise + (K + o) * 256 + 8 * g, e);
        const uint32_t mb = o < K ? 0u : (uint32_t)m[g];
        uint32_t acc = 0;
        int nb = 0, pos = at;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const int32_t ei = (int16_t)e[i];
            const uint32_t v = (mulq(x[i], INV128) + (uint32_t)(ei + ((ei >> 31) & Q)) + ((mb >> i) & 1u) * (uint32_t)((Q + 1) / 2)) % (uint32_t)Q;
            acc |= compress(v, d) << nb;
            nb += d;
            while (nb >= 8) { // d and nb are public
                const uint32_t byte = acc & 0xFF;
                if (ct_out) ct_out[pos] = (uint8_t)byte;
                else diff |= byte ^ (uint32_t)ct_cmp[pos];
                pos++;
                acc >>= 8;
                nb -= 8;
            }
        }
    }
    return diff;
}

// --------------------------------------------------------------------------------------------------- indcpa_dec --
// LDS tile L: (K + 2) polynomials -- u[K] | v | mp; Lb: 288 bytes (256 message bits, then the 32 message bytes).
// m' goes to Lb + 256 (and, by the caller, wherever it is needed).  sk: 384 K bytes of s-hat.
KOSK_HD inline void decrypt_block(const Dims &D, uint16_t *L, uint8_t *Lb, int tid, int nthr, const uint8_t *ct, const uint8_t *sk)
{
    const int K = D.K;
    uint16_t *V = L + K * 256, *MP = L + (K + 1) * 256;
    for (int w = tid; w < (K + 1) * 32; w += nthr) {
        const int o = w >> 5, g = w & 31, d = o < K ? D.du : D.dv;
        const uint8_t *p = ct + (o < K ? (o * 32 + g) * D.du : D.ub + g * D.dv);
        uint32_t acc = 0, c[8];
        int nb = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) {
            while (nb < d) { acc |= (uint32_t)(*p++) << nb; nb += 8; }
            c[i] = decompress(acc & ((1u << d) - 1u), d);
            acc >>= d;
            nb -= d;
        }
        store16x8(L + o * 256 + 8 * g, c);
    }
    KEM_SYNC();
    ntt_tile(L, K, tid, nthr);
    for (int g = tid; g < 32; g += nthr) {
        uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int j = 0; j < K; j++) {
            uint32_t a[8], b[8];
            load12x8(sk + j * 384 + 12 * g, a);
            load16x8(L + j * 256 + 8 * g, b);
            basemul8_acc(acc, a, b, g);
        }
        store16x8(MP + 8 * g, acc);
    }
    KEM_SYNC();
    invntt_tile(MP, 1, tid, nthr);
    for (int c = tid; c < 256; c += nthr) {
        const uint32_t x = csub((uint32_t)V[c] + (uint32_t)Q - mulq(MP[c], INV128));
        Lb[c] = (uint8_t)compress(x, 1);
    }
    KEM_SYNC();
    for (int i = tid; i < 32; i += nthr) {
        uint32_t byte = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) byte |= (uint32_t)Lb[8 * i + j] << j;
        Lb[256 + i] = (uint8_t)byte;
    }
    KEM_SYNC();
}

// ------------------------------------------------------------------------------------------- indcpa_keypair_derand --
// (rho, sigma) = hash_g (sha3_512) of d[32] || K (indcpa.c:219-221): 33 bytes, rate 72
KOSK_HD inline void seed_hash_g(const uint64_t (&d)[4], int K, uint64_t (&out)[8])
{
    uint64_t s[25];
    zero(s);
#pragma unroll
    for (int l = 0; l < 4; l++) s[l] = d[l];
    s[4] = (uint64_t)(uint32_t)K | (0x06ULL << 8);
    s[8] = 0x8000000000000000ULL;
    perm(s);
#pragma unroll
    for (int l = 0; l < 8; l++) out[l] = s[l];
}

// One workgroup, one key pair (indcpa.c:231-244, kem.c:29-33).  LDS tile L: 2 K polynomials of 256 u16 -- s-hat[K] | e-hat[K], then
// t-hat[K] in e-hat's place; Lb: the sk record (768 K + 96 bytes, 16-byte aligned) as it will stand, its H(pk) field zero.
//   A     : A[K][K][256] int16 in [0, q), row-major as multiplied (t-hat_i = sum_j A[i][j] o s-hat_j), 16-byte aligned
//   noise : s[K] | e[K], int16[256] each, 16-byte aligned             rho, z : 32 bytes each, 4-byte aligned
// tomont cancels the Montgomery factor of the reference's base multiplication, so on residues t-hat = A o s-hat + e-hat.
// pk_out and sk_out (16-byte aligned) receive whole records in 16-byte stores; the caller's hash fills sk_out's H(pk) afterwards.
// Secrets: s, e, s-hat and z are data only; every address is a function of the thread index.
KOSK_HD inline void keypair_block(const Dims &D, uint16_t *L, uint8_t *Lb, int tid, int nthr, const int16_t *A, const int16_t *noise,
                                  const uint8_t *rho, const uint8_t *z, uint8_t *pk_out, uint8_t *sk_out)
{
    const int K = D.K;
    for (int w = tid; w < 2 * K * 32; w += nthr) {
        uint32_t c[8];
        load16x8(noise + 8 * w, c);
#pragma unroll
        for (int i = 0; i < 8; i++) { const int32_t e = (int16_t)c[i]; c[i] = (uint32_t)(e + ((e >> 31) & Q)); }
        store16x8(L + 8 * w, c);
    }
    KEM_SYNC();
    ntt_tile(L, 2 * K, tid, nthr);
    // t-hat_i over e-hat_i: group (i, g) of e-hat is read and written by this work item alone, s-hat is only read
    for (int w = tid; w < K * 32; w += nthr) {
        const int i = w >> 5, g = w & 31;
        uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, e[8];
        for (int j = 0; j < K; j++) {
            uint32_t a[8], b[8];
            load16x8(A + ((i * K + j) * 256 + 8 * g), a);
            load16x8(L + j * 256 + 8 * g, b);
            basemul8_acc(acc, a, b, g);
        }
        load16x8(L + (K + i) * 256 + 8 * g, e);
#pragma unroll
        for (int c = 0; c < 8; c++) acc[c] = csub(acc[c] + e[c]);
        store16x8(L + (K + i) * 256 + 8 * g, acc);
    }
    KEM_SYNC();
    // sk = tobytes(s-hat) || tobytes(t-hat) || rho || H(pk) || z: polynomial o of the tile is bytes 384 o .. of the record
    for (int w = tid; w < 2 * K * 32; w += nthr) {
        uint32_t c[8];
        load16x8(L + 8 * w, c);
        store12x8(Lb + 12 * w, c);
    }
    for (int i = tid; i < 8; i += nthr) {
        uint32_t *tail = reinterpret_cast<uint32_t *>(Lb + 2 * D.pvb);
        tail[i] = reinterpret_cast<const uint32_t *>(rho)[i];
        tail[8 + i] = 0;
        tail[16 + i] = reinterpret_cast<const uint32_t *>(z)[i];
    }
    KEM_SYNC();
    for (int i = tid; i < D.sk / 16; i += nthr) reinterpret_cast<U128 *>(sk_out)[i] = reinterpret_cast<const U128 *>(Lb)[i];
    for (int i = tid; i < D.pk / 16; i += nthr) reinterpret_cast<U128 *>(pk_out)[i] = reinterpret_cast<const U128 *>(Lb + D.pvb)[i];
}

// ------------------------------------------------------------------------------------------------------ key checks --
// non-zero iff one of the eight 12-bit fields at the 4-byte aligned p is >= q (FIPS 203 7.2): the sign bits of q - 1 - c, no branch
KOSK_HD inline uint32_t range12x8(const uint8_t *p)
{
    uint32_t c[8], bad = 0;
    unpack12x8(p, c);
#pragma unroll
    for (int i = 0; i < 8; i++) bad |= ((uint32_t)(Q - 1) - c[i]) >> 31;
    return bad;
}
// 1 iff x != 0, for x < 2^24, without a branch
KOSK_HD inline uint32_t nonzero_bit(uint32_t x) { return ((x + 0xFFFFFFu) >> 24) & 1u; }

// ss = fail ? rk : kbar without a branch: `diff` is the OR of all byte differences (0 .. 255)
KOSK_HD inline uint8_t select_ss(uint32_t diff, uint8_t kbar, uint8_t rk)
{
    const uint32_t equal_mask = ((diff + 0xFFu) >> 8) - 1u; // all ones iff diff == 0
    return (uint8_t)(rk ^ (equal_mask & (uint32_t)(rk ^ kbar)));
}

} // namespace kem
} // namespace kosk
