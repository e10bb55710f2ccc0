// The Cauchy-product engine under k_interp_apply / k_gather_frags (kosk_verify_kernels.hip) and k_dense_fill (kosk_dense.hip): both
// apply a per-proof barycentric interpolation operator, out[i][c] = l_i * sum_j 1/(x_i - x_j) * (w_j y[j][c]), as an int8-limb MFMA
// product without storing it.  The weighted shares w_j y[j][c] are a limb matrix of fragment-linear tiles (kosk_device.hpp: frag_offset
// with r = column, k = node, RT = column tiles); the operand 1/(x_i - x_j) is built by every lane in registers from the ascending node
// list and a table of limb pairs (kosk_device.hpp: limb_pair), both in LDS.  This header owns everything between "nodes, table and weighted
// shares are in place" and "the accumulators hold the Cauchy sums"; the kernels keep their work distribution, the origin of table and shares, their epilogues.
#pragma once
#include "kosk_limb_dev.hpp"

namespace kosk {

// a b mod q for a, b < 2^16 with a b < 2^32 in seven full-rate instructions (24-bit multiply + gf_reduce_u32) where `a * b % Q` costs three
// quarter-rate 32-bit multiplies; the canonical representative of a difference |d| < q; a^(q-2) (0 -> 0)
__device__ __forceinline__ uint32_t gf_mul_fast(uint32_t a, uint32_t b) { return gf_reduce_u32(__umul24(a, b)); }
__device__ __forceinline__ uint32_t gf_diff(int d) { return (uint32_t)(d < 0 ? d + Q : d); }
__device__ __forceinline__ uint32_t gf_inv_pow(uint32_t a)
{
    uint32_t r = 1, b = a;
#pragma unroll 1
    for (int e = Q - 2; e; e >>= 1) {
        if (e & 1) r = gf_mul_fast(r, b);
        b = gf_mul_fast(b, b);
    }
    return r;
}

// One fragment of the weighted shares: column r, the sixteen nodes from 16 kc16 on.  fetch(y, w) delivers their values y (any u16) and
// weights w (< q) and is only called where `live`; a dead fragment is zero.  Two 16-byte stores.
template <class Fetch>
__device__ __forceinline__ void cauchy_weighted_frag(uint8_t *tiles, int r, int kc16, int NT, bool live, Fetch &&fetch)
{
    uint32_t o[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (live) {
        uint32_t y[16], w[16];
        fetch(y, w);
#pragma unroll
        for (int q = 0; q < 16; q += 2) o[q >> 1] = gf_mul_fast(w[q], y[q]) | (gf_mul_fast(w[q + 1], y[q + 1]) << 16);
    }
    uint4 lo, hi;
    gm_split16(make_uint4(o[0], o[1], o[2], o[3]), make_uint4(o[4], o[5], o[6], o[7]), lo, hi);
    *reinterpret_cast<uint4 *>(tiles + frag_offset(r, kc16 * 16, 0, NT)) = lo;
    *reinterpret_cast<uint4 *>(tiles + frag_offset(r, kc16 * 16, 1, NT)) = hi;
}

// The operand fragment of k-step ks: row = the lane's evaluation point (lane & 15), k = its sixteen nodes j = 64 ks + 16 (lane >> 4) + q;
// the limbs of 1/(x - x_j) come from tab_s[kq - rest_s[j]] (kq: the point plus the table's offset) and are split into low limbs a0 and high
// limbs a1 with two v_perm per dword.  CLAMP != 0: indices are clamped to CLAMP, an entry that holds 0 (a list that was not validated)
template <uint32_t CLAMP>
__device__ __forceinline__ void cauchy_operand_frag(const uint16_t *rest_s, const uint16_t *tab_s, int ks, int lane, int kq, v4i &a0, v4i &a1)
{
    const uint16_t *rn = rest_s + ks * 64 + (lane >> 4) * 16;
    const uint4 r0 = *reinterpret_cast<const uint4 *>(rn), r1 = *reinterpret_cast<const uint4 *>(rn + 8);
    const uint32_t rw[8] = {r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, r1.w};
    uint32_t e[16];
#pragma unroll
    for (int q = 0; q < 16; q++) {
        const int xj = (int)((rw[q >> 1] >> (16 * (q & 1))) & 0xFFFFu);
        e[q] = tab_s[CLAMP ? min((uint32_t)(kq - xj), CLAMP) : (uint32_t)(kq - xj)];
    }
    uint32_t lo[4], hi[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const uint32_t t01 = e[4 * q] | (e[4 * q + 1] << 16), t23 = e[4 * q + 2] | (e[4 * q + 3] << 16);
        lo[q] = __builtin_amdgcn_perm(t23, t01, 0x06040200u);
        hi[q] = __builtin_amdgcn_perm(t23, t01, 0x07050301u);
    }
    a0 = (v4i){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3]};
    a1 = (v4i){(int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}

// The Cauchy sums of one wave: 16 evaluation points x 16 NT columns over 64 KS nodes, as the three limb products
// a0 b0 -> s0, a0 b1 + a1 b0 -> s1, a1 b1 -> s2.  D[row = point 4 (lane >> 4) + r][col = 16 j + (lane & 15)] = value(j, r).
// The other operand comes from a loader: ld.frag(ks, j, limb) returns the lane's fragment of the weighted shares (16 bytes at 16 lane
// of the tile), ld.ahead(ks) is called at the head of k-step ks and once with ks = -1 in front of the loop (a loader that prefetches
// starts the loads of k-step ks + 1 there).
template <int KS, int NT>
struct CauchySums {
    static_assert(KS * 64 <= 832, "gf_reduce_limbs' bias covers 13 k-steps");
    v4i s0[NT], s1[NT], s2[NT];

    template <uint32_t CLAMP, class Loader>
    __device__ __forceinline__ void run(const uint16_t *rest_s, const uint16_t *tab_s, int lane, int kq, Loader &ld)
    {
#pragma unroll
        for (int j = 0; j < NT; j++) { s0[j] = (v4i){0, 0, 0, 0}; s1[j] = s0[j]; s2[j] = s0[j]; }
        ld.ahead(-1);
#pragma unroll
        for (int ks = 0; ks < KS; ks++) {
            ld.ahead(ks);
            v4i a0, a1;
            cauchy_operand_frag<CLAMP>(rest_s, tab_s, ks, lane, kq, a0, a1);
#pragma unroll
            for (int j = 0; j < NT; j++) {
                const v4i b0 = ld.frag(ks, j, 0), b1 = ld.frag(ks, j, 1);
                s0[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b0, s0[j], 0, 0, 0);
                s1[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b1, s1[j], 0, 0, 0);
                s2[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b1, s2[j], 0, 0, 0);
                s1[j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b0, s1[j], 0, 0, 0);
            }
        }
    }
    __device__ __forceinline__ uint32_t value(int j, int r) const { return gf_reduce_limbs(s0[j][r], s1[j][r], s2[j][r]); }
};

} // namespace kosk
