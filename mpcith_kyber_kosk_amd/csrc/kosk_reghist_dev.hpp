// Device code that the history's two tier-0 kernels share: k_reghist_append (kosk_reghist.hip) forms its leaves from
// (op, slot, h[slot]) or the two roots, k_monitor_leaves (kosk_monitor.hip) from stored event records; the levels above are one function.
#pragma once
#include <hip/hip_runtime.h>

#include "kosk_ctx.hpp"
#include "kosk_kem_dev.hpp"
#include "kosk_reghist.hpp"

namespace kosk {

__device__ __forceinline__ kem::U128 words_u128(uint64_t a, uint64_t b) { return kem::U128{(uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)}; }
__device__ __forceinline__ void reghist_store(uint8_t *dst, const uint64_t (&d)[4])
{
    kem::U128 *o = reinterpret_cast<kem::U128 *>(dst);
    o[0] = words_u128(d[0], d[1]);
    o[1] = words_u128(d[2], d[3]);
}
__device__ __forceinline__ void reghist_load(const uint8_t *src, uint64_t (&d)[4])
{
    const kem::U128 a = reinterpret_cast<const kem::U128 *>(src)[0], b = reinterpret_cast<const kem::U128 *>(src)[1];
    d[0] = (uint64_t)a.x | (uint64_t)a.y << 32; d[1] = (uint64_t)a.z | (uint64_t)a.w << 32;
    d[2] = (uint64_t)b.x | (uint64_t)b.y << 32; d[3] = (uint64_t)b.z | (uint64_t)b.w << 32;
}

// The group of a tier that block blockIdx.x owns: lo = its first input, cnt = how many of the level's complete nodes (after the append) it
// holds, in_lvl = where input lo lies
struct RegHistGroup {
    int L0, lo, cnt, up;
    uint8_t *in_lvl;
};
__device__ __forceinline__ RegHistGroup reghist_group(const RegHistAppendJob &j)
{
    RegHistGroup g;
    g.L0 = j.tier * reghist::TIER_LEVELS;
    const int so = j.s >> g.L0, ne = (j.s + j.c) >> g.L0;
    g.lo = ((so >> reghist::TIER_LEVELS) + (int)blockIdx.x) << reghist::TIER_LEVELS;
    g.cnt = ne - g.lo < (int)reghist::TIER_INPUTS ? ne - g.lo : (int)reghist::TIER_INPUTS;
    g.up = j.D - g.L0 < (int)reghist::TIER_LEVELS ? j.D - g.L0 : (int)reghist::TIER_LEVELS;
    g.in_lvl = j.nodes + regtree::level_offset(j.D, g.L0) + (size_t)g.lo * 32;
    return g;
}

// The levels above a group's inputs, which lie in lds[0 .. 4 cnt) behind a barrier.  Node i of level lv above (numbered from the group's
// first) is fresh iff it became complete with this append; a node that was complete before is loaded, for the level above may need it.
// All loop bounds are block-uniform.  lds: (TIER_INPUTS + TIER_INPUTS / 2) * 4 words
__device__ __forceinline__ void reghist_levels(const RegHistAppendJob &j, const RegHistGroup &g, uint64_t *lds)
{
    const int tid = threadIdx.x;
    int in = 0, out = reghist::TIER_INPUTS * 4; // word offsets of the two buffers
    for (int lv = 1; lv <= g.up && (g.cnt >> lv); lv++) {
        const int m = g.cnt >> lv;
        const size_t first = (size_t)g.lo >> lv;
        uint8_t *dst = j.nodes + regtree::level_offset(j.D, g.L0 + lv) + first * 32;
        for (int i = tid; i < m; i += 256) {
            uint64_t l[4];
            if (((uint64_t)(first + i + 1) << (g.L0 + lv)) > (uint64_t)j.s) {
                uint64_t r[4], st[25];
#pragma unroll
                for (int w = 0; w < 4; w++) { l[w] = lds[in + 8 * i + w]; r[w] = lds[in + 8 * i + 4 + w]; }
                reghist::node_state(st, l, r);
                kem::perm(st);
#pragma unroll
                for (int w = 0; w < 4; w++) l[w] = st[w];
                reghist_store(dst + (size_t)i * 32, l);
            } else {
                reghist_load(dst + (size_t)i * 32, l);
            }
#pragma unroll
            for (int w = 0; w < 4; w++) lds[out + 4 * i + w] = l[w];
        }
        __syncthreads();
        const int t = in; in = out; out = t;
    }
}

} // namespace kosk
