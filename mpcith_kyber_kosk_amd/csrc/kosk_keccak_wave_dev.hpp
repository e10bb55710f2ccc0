// Wave-cooperative Keccak sponge: ONE Keccak-f[1600] state per 64-lane wave, one 32-bit word per lane.
// (kosk_keccak_dev.hpp: one state per lane; kosk_keccak_split_dev.hpp: one state per lane pair.)
//
// Why: the Fiat-Shamir aggregation hashes sha3_256(Tcomm[0..1454)) and sha3_256(ch_seeds) (mlwe_prover.cpp:130-135, :445-449;
// mlwe_verifier.cpp:40-44, :648-652) are ONE sequential chain of 343 permutations per proof and round (sha3_256_long of SURVEY.md
// 2.1 K4b).  The pipeline's one-state-per-lane sponge needs ~9 us per permutation when a wave runs alone (180 instructions per
// round at one issue slot per ~5 cycles): 3 ms per chain.  Here every vector instruction acts on the WHOLE state, and
// no exchange goes through LDS memory:
//
//   lane(x, y, h) = 32 h + (x < 3 ? 5 x : 16 + 5 (x - 3)) + y  holds half h (0: even bits, 1: odd bits of the bit-interleaved form)
//   of the 64-bit word (x, y): columns of FIVE lanes that never straddle a 16-lane row.  The idle lanes (15, 26..31 of each half)
//   hold junk no active lane ever reads.
//   theta   c = the column's sum, three DPP-fused xors (row_shr:1, :2, :1; it lands on the lane y = 4);  Cm, Cp = the sums of
//           columns x - 1 (this half) and x + 1 (OTHER half), one ds_bpermute_b32 gather each;
//           a ^= Cm ^ rotl32(Cp, h == 0)                (rotl64 by 1, interleaved: E' = rotl32(O, 1), O' = E)
//   rho     a = rotl32(a, k)                            64-bit offset r: k = r >> 1 (+1 on the odd half when r is odd; the halves
//                                                       change places when r is odd, which the pi gather addresses absorb)
//   pi/chi  (b0, b1, b2) = three gathers: the pre-images of words x, x + 1, x + 2 of the lane's row, rotated by their owners
//           before they are sent;  a = b0 ^ (~b1 & b2) ^ rc      chi is one v_bitop3, iota one xor with a per-lane register
//
// A variant with both exchanges through LDS memory was measured 4 % slower and removed (profiles/r06_fs_device.txt).
// tools/fs_chain_model.py is the lane-level model of exactly these tables and exchanges (checked against hashlib in the CPU suite).
// Semantics: kyber/fips202.c:82-344 (KeccakF1600_StatePermute), :461-485 (absorb / squeeze), :745-754 (sha3_256).
#pragma once
#include <hip/hip_runtime.h>

#include "kosk_keccak_dev.hpp"
#include "kosk_wave_sync_dev.hpp"

namespace kosk {

// even bits (sel 0) or odd bits (sel 1) of the 64-bit value hi:lo
__device__ __forceinline__ uint32_t fs_deinterleave_half(uint32_t lo, uint32_t hi, uint32_t sel)
{
    uint32_t a = (lo >> sel) & 0x55555555u, b = (hi >> sel) & 0x55555555u;
    a = (a | (a >> 1)) & 0x33333333u; b = (b | (b >> 1)) & 0x33333333u;
    a = (a | (a >> 2)) & 0x0F0F0F0Fu; b = (b | (b >> 2)) & 0x0F0F0F0Fu;
    a = (a | (a >> 4)) & 0x00FF00FFu; b = (b | (b >> 4)) & 0x00FF00FFu;
    a = (a | (a >> 8)) & 0x0000FFFFu; b = (b | (b >> 8)) & 0x0000FFFFu;
    return a | (b << 16);
}
__device__ __forceinline__ uint32_t fs_spread16(uint32_t v) // bit i of the low 16 bits -> bit 2 i
{
    v &= 0xFFFFu;
    v = (v | (v << 8)) & 0x00FF00FFu;
    v = (v | (v << 4)) & 0x0F0F0F0Fu;
    v = (v | (v << 2)) & 0x33333333u;
    v = (v | (v << 1)) & 0x55555555u;
    return v;
}
// the 64-bit word whose even bits are e and whose odd bits are o
__device__ __forceinline__ void fs_interleave(uint32_t e, uint32_t o, uint32_t &lo, uint32_t &hi)
{
    lo = fs_spread16(e) | (fs_spread16(o) << 1);
    hi = fs_spread16(e >> 16) | (fs_spread16(o >> 16) << 1);
}

// this lane's half of the 24 round constants (zero everywhere but on the two lanes of word (0, 0))
struct FsRc {
    uint32_t v[24];
};
__device__ __forceinline__ FsRc fs_rc_setup(uint32_t half, int word)
{
    FsRc rc;
#pragma unroll
    for (int r = 0; r < 24; r++) {
        const uint64_t c = kKeccakRcDev[r];
        const uint32_t mine = fs_deinterleave_half((uint32_t)c, (uint32_t)(c >> 32), half);
        rc.v[r] = word == 0 ? mine : 0u;
    }
    return rc;
}

// the rho offset of word (x, y) by the walk of FIPS 202 3.2.2 (once per kernel; equals kRho[x + 5 y] of kosk_math.hpp)
__device__ __forceinline__ int fs_rho_of(int x, int y)
{
    int rot = 0;
    for (int t = 0, wx = 1, wy = 0; t < 24; t++) {
        if (wx == x && wy == y) rot = ((t + 1) * (t + 2) / 2) & 63;
        const int nx = wy, ny = (2 * wx + 3 * wy) % 5;
        wx = nx; wy = ny;
    }
    return rot;
}

template <int CTRL>
__device__ __forceinline__ uint32_t fs_dpp_xor(uint32_t moved, uint32_t other) // dpp(moved) ^ other, one v_xor_b32_dpp
{
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)moved, CTRL, 0xF, 0xF, true) ^ other;
}

// The sponge of one wave: `a`, the lane's word of the state, stays with the caller.  All 64 lanes must be active in every member.
struct WaveSponge {
    struct Lane {
        uint32_t sCm, sCp, s0, s1, s2; // byte addresses (lane * 4) for ds_bpermute_b32
        uint32_t sh_theta, sh_rho;     // v_alignbit shift amounts (rotate right by sh = rotate left by 32 - sh)
        uint32_t half;                 // 0 even bits, 1 odd bits
        int word;                      // x + 5 y of an active lane, 63 for an idle one
    };
    Lane L;
    FsRc rc;
    int lane;

    static __device__ __forceinline__ int lane_of(int x, int y, int h) { return 32 * h + (x < 3 ? 5 * x : 16 + 5 * (x - 3)) + y; }
    __device__ __forceinline__ uint32_t half() const { return L.half; }
    __device__ __forceinline__ int word() const { return L.word; }

    static __device__ __forceinline__ Lane lane_setup(int lane)
    {
        Lane L;
        const int h = lane >> 5, r = lane & 31;
        const int x = r < 15 ? r / 5 : r >= 16 && r < 26 ? 3 + (r - 16) / 5 : 5;
        const int y = r < 15 ? r % 5 : r >= 16 && r < 26 ? (r - 16) % 5 : 0;
        L.half = (uint32_t)h;
        if (x >= 5) {
            L.word = 63;
            L.sCm = L.sCp = L.s0 = L.s1 = L.s2 = (uint32_t)lane * 4;
            L.sh_theta = L.sh_rho = 0;
            return L;
        }
        L.word = x + 5 * y;
        L.sCm = 4u * (uint32_t)lane_of((x + 4) % 5, 4, h);
        L.sCp = 4u * (uint32_t)lane_of((x + 1) % 5, 4, 1 - h);
        L.sh_theta = h == 0 ? 31u : 0u;
        const int rot = fs_rho_of(x, y);
        const int k = (rot >> 1) + (((rot & 1) && h == 1) ? 1 : 0);
        L.sh_rho = (uint32_t)((32 - k) & 31);
        uint32_t src[3];
        for (int j = 0; j < 3; j++) { // word (x + j, y) of the permuted state sits, rotated, on the lane of its pre-image under pi
            const int X = (x + j) % 5, Y = y, ys = X, xs = (3 * (Y - 3 * X + 15)) % 5, hs = h ^ (fs_rho_of(xs, ys) & 1);
            src[j] = 4u * (uint32_t)lane_of(xs, ys, hs);
        }
        L.s0 = src[0]; L.s1 = src[1]; L.s2 = src[2];
        return L;
    }
    __device__ __forceinline__ void setup(int lane_)
    {
        lane = lane_;
        L = lane_setup(lane_);
        rc = fs_rc_setup(L.half, L.word);
    }

    // Keccak-f[1600] on the wave's state
    __device__ __forceinline__ void permute(uint32_t &a) const
    {
#pragma unroll
        for (int r = 0; r < 24; r++) {
            const uint32_t t1 = fs_dpp_xor<0x111>(a, a);   // row_shr:1
            const uint32_t t2 = fs_dpp_xor<0x112>(t1, t1); // row_shr:2
            const uint32_t c = fs_dpp_xor<0x111>(t2, a);   // the column's sum on its lane y = 4
            const uint32_t cm = (uint32_t)__builtin_amdgcn_ds_bpermute((int)L.sCm, (int)c);
            const uint32_t cp = (uint32_t)__builtin_amdgcn_ds_bpermute((int)L.sCp, (int)c);
            a = kx3(a, cm, __builtin_amdgcn_alignbit(cp, cp, L.sh_theta));
            a = __builtin_amdgcn_alignbit(a, a, L.sh_rho);
            const uint32_t b0 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)L.s0, (int)a);
            const uint32_t b1 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)L.s1, (int)a);
            const uint32_t b2 = (uint32_t)__builtin_amdgcn_ds_bpermute((int)L.s2, (int)a);
            a = kchi(b0, b1, b2) ^ rc.v[r];
        }
    }

    // XOR this lane's word m (standard form, zero on the lanes beyond the rate) of a message block into the state
    __device__ __forceinline__ void absorb(uint32_t &a, uint2 m) const { a ^= fs_deinterleave_half(m.x, m.y, L.half); }

    // The padding as word `w` of the last block sees it: the domain byte behind the `len` bytes absorbed into that block, 0x80 on the
    // last byte of the rate (both in bytes; len < rate).  What the message itself puts into the same word is the caller's to add.
    static __device__ __forceinline__ uint2 pad(int w, int len, uint32_t dom, int rate)
    {
        uint32_t lo = 0, hi = 0;
        if ((len >> 3) == w) {
            const int sh = 8 * (len & 7);
            if (sh < 32) lo = dom << sh;
            else hi = dom << (sh - 32);
        }
        if (w == rate / 8 - 1) hi ^= 0x80000000u;
        return make_uint2(lo, hi);
    }

    // Words 0..n-1 of the state in standard form on the lanes 0..n-1 (zero on the others), through the caller's 64 words of LDS.
    // The handoffs on both sides of the store are here: st may have been read just before (by an earlier call), and is read right after.
    __device__ __forceinline__ uint2 words(uint32_t a, uint32_t *st, int n) const
    {
        uint2 w = make_uint2(0, 0);
        wave_lds_handoff();
        st[lane] = a;
        wave_lds_handoff();
        if (lane < n) {
            const int x = lane % 5, y = lane / 5;
            fs_interleave(st[lane_of(x, y, 0)], st[lane_of(x, y, 1)], w.x, w.y);
        }
        return w;
    }
};

// The whole-word message of a wave sponge at rate 136 (17 words a block): absorbs words fetch(0 .. nwords - 1) and the padding behind them,
// domain byte `dom` (0x06 SHA3, 0x1F SHAKE), through the last permutation.  Which word a lane fetches is a function of the lane and the block.
template <class Fetch>
__device__ __forceinline__ void wave_absorb_words(const WaveSponge &sp, uint32_t &a, Fetch fetch, int nwords, uint32_t dom)
{
    const int word = sp.word(), nfull = nwords / 17, rem = nwords - 17 * nfull;
    for (int blk = 0; blk < nfull; blk++) {
        sp.absorb(a, word < 17 ? fetch(17 * blk + word) : make_uint2(0, 0));
        sp.permute(a);
    }
    // rem <= 16 whole words, then the padding: the domain byte opens the first free word
    sp.absorb(a, word < rem ? fetch(17 * nfull + word) : WaveSponge::pad(word, 8 * rem, dom, 136));
    sp.permute(a);
}

} // namespace kosk
