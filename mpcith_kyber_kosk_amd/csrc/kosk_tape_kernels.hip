// Seeded proving: randomness tapes from 32-byte seeds (format kosk-seedtape-v1; no reference counterpart: the
// reference draws every tape byte through randombytes, kosk.cpp:12, mlwe_prover.cpp:9, ss.cpp:5).
//   block_j = SHAKE256(seed[32] || "kosk-seedtape-v1" || LE32(K) || LE32(j))[0:136],   tape = (block_0 || block_1 || ...)[0:T]
//   k_tape_expand    n x NB independent single-permutation sponges, one per thread; the 64 blocks of a wave are 8 704 contiguous
//                    tape bytes, staged through LDS and written 16 bytes per lane, consecutive lanes consecutive
#include <hip/hip_runtime.h>

#include "kosk_device.hpp"
#include "kosk_keccak_dev.hpp"
#include "kosk_math.hpp"

namespace kosk {

constexpr int TAPE_RATE = 136;                  // SHAKE256 rate: one block per permutation
constexpr int TAPE_WAVE_BYTES = 64 * TAPE_RATE; // what the 64 sponges of a wave produce
// "kosk-seedtape-v1" as two little-endian lanes
constexpr uint64_t TAPE_LABEL0 = 0x6565732d6b736f6bULL; // "kosk-see"
constexpr uint64_t TAPE_LABEL1 = 0x31762d6570617464ULL; // "dtape-v1"

// `len` bytes of the wave's LDS image, from byte `o` (a multiple of 8) on, to dst (a multiple of 8): an 8-byte head where dst is not
// a multiple of 16, then 16 bytes per lane, then the tail of a truncated last block byte by byte.  All arguments are wave-uniform.
__device__ __forceinline__ void tape_store_segment(uint8_t *__restrict__ dst, const uint8_t *lds, int o, int len, int lane)
{
    if ((reinterpret_cast<uintptr_t>(dst) & 15) && len >= 8) {
        if (lane == 0) *reinterpret_cast<uint64_t *>(dst) = *reinterpret_cast<const uint64_t *>(lds + o);
        dst += 8; o += 8; len -= 8;
    }
    const int nvec = len >> 4;
    for (int i = lane; i < nvec; i += 64) {
        const uint64_t *s = reinterpret_cast<const uint64_t *>(lds + o + 16 * i);
        ulonglong2 v;
        v.x = s[0];
        v.y = s[1];
        *reinterpret_cast<ulonglong2 *>(dst + 16 * (size_t)i) = v;
    }
    const int done = nvec << 4;
    if (lane < len - done) dst[done + lane] = lds[o + done + lane];
}

// sponge g = b * NB + j writes tape bytes [136 j, min(136 (j + 1), T)) of proof b.  One wave per workgroup: sponges [64 w, 64 w + 64),
// which lie in at most two proofs (NB >= 480).
__global__ __launch_bounds__(64) void k_tape_expand(const uint8_t *__restrict__ seeds, size_t seed_stride, uint8_t *__restrict__ tapes,
                                                    size_t tape_stride, int K, int T, int NB, int n)
{
    __shared__ __attribute__((aligned(16))) uint8_t img[TAPE_WAVE_BYTES];
    const int lane = threadIdx.x;
    const long total = (long)n * NB;
    const long g0 = (long)blockIdx.x * 64;
    const int b0 = (int)(g0 / NB), j0 = (int)(g0 - (long)b0 * NB);
    const int first = NB - j0 < 64 ? NB - j0 : 64; // sponges of this wave that belong to proof b0
    // the (at most two) seeds of the wave: uniform addresses, read once per wave
    const int b1 = b0 + 1 < n ? b0 + 1 : b0;
    const uint64_t *sa = reinterpret_cast<const uint64_t *>(seeds + (size_t)b0 * seed_stride);
    const uint64_t *sb = reinterpret_cast<const uint64_t *>(seeds + (size_t)b1 * seed_stride);
    const bool second = lane >= first;
    const int j = second ? lane - first : j0 + lane;
    // the tapes head a run's dependency chain (k_prover_pre reads them) and the grid is two waves per SIMD: like the other sponge kernels
    // on that chain, do not queue behind the bulk kernels of the cohorts that share the chip
    __builtin_amdgcn_s_setprio(3);
    KState s;
    kstate_zero(s);
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint64_t v = second ? sb[i] : sa[i];
        s.lo[i] = (uint32_t)v;
        s.hi[i] = (uint32_t)(v >> 32);
    }
    s.lo[4] = (uint32_t)TAPE_LABEL0; s.hi[4] = (uint32_t)(TAPE_LABEL0 >> 32);
    s.lo[5] = (uint32_t)TAPE_LABEL1; s.hi[5] = (uint32_t)(TAPE_LABEL1 >> 32);
    s.lo[6] = (uint32_t)K; s.hi[6] = (uint32_t)j;
    s.lo[7] = 0x1F;         // SHAKE domain byte at byte 56
    s.hi[16] = 0x80000000u; // end of the pad at byte 135
    keccak_f1600_dev(s);
    uint64_t *mine = reinterpret_cast<uint64_t *>(img + lane * TAPE_RATE);
#pragma unroll
    for (int i = 0; i < 17; i++) mine[i] = (uint64_t)s.lo[i] | ((uint64_t)s.hi[i] << 32);
    __syncthreads();
    // proof b0: blocks j0 .. j0 + first - 1, cut at T
    {
        const int off = j0 * TAPE_RATE;
        int len = first * TAPE_RATE;
        if (off + len > T) len = T - off;
        tape_store_segment(tapes + (size_t)b0 * tape_stride + off, img, 0, len, lane);
    }
    // proof b0 + 1: blocks 0 .. (the wave's other sponges), where it exists
    const long rest = total - (g0 + first);
    if (first < 64 && rest > 0) {
        const int cnt = rest < 64 - first ? (int)rest : 64 - first;
        int len = cnt * TAPE_RATE;
        if (len > T) len = T;
        tape_store_segment(tapes + (size_t)(b0 + 1) * tape_stride, img, first * TAPE_RATE, len, lane);
    }
}

hipError_t launch_tape_expand(const uint8_t *seeds, size_t seed_stride, uint8_t *tapes, size_t tape_stride, int K, int tape_bytes, int n,
                              hipStream_t st)
{
    const int NB = (tape_bytes + TAPE_RATE - 1) / TAPE_RATE;
    const long total = (long)n * NB;
    hipLaunchKernelGGL(k_tape_expand, dim3((unsigned)((total + 63) / 64)), dim3(64), 0, st, seeds, seed_stride, tapes, tape_stride, K,
                       tape_bytes, NB, n);
    return hipGetLastError();
}

} // namespace kosk
