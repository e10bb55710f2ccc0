// The prover's witness from an existing Kyber secret key, on gfx950: one workgroup per key record
//   sk = NTT(s) bytes || pk || H(pk) || z      (kosk.cpp:62-69; H(pk) and z are not read)
// -> s = NTT^-1(s-hat), e = NTT^-1(t-hat - A o s-hat) as centred int16 where the prover's first launch reads its witness, the range
// verdict, and the embedded pk bytes where the key generation leaves them.  A and t-hat come from launch_decode_pk on the embedded pk
// (kosk_keygen_kernels.hip), queued ahead of this kernel on the same stream.  The 2 K polynomials of a key go through the inverse NTT as
// ONE tile in LDS (4 KB for K = 4); the device functions are in kosk_witness_dev.hpp, DESIGN.md 21 has the resource figures.
#include <hip/hip_runtime.h>

#include "kosk_device.hpp"
#include "kosk_witness_dev.hpp"

namespace kosk {

using namespace wit;

__global__ __launch_bounds__(256) void k_witness_from_sk(WitnessArgs a)
{
    __shared__ alignas(16) uint16_t L[8 * 256];
    __shared__ uint32_t bad_all;
    const Dims D = dims(a.K);
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const uint8_t *sk = a.sk + b * a.sk_stride;
    if (tid == 0) bad_all = 0;
    __syncthreads();
    const uint32_t bad = recover_block(D, L, tid, 256, sk, a.A + b * a.A_stride, a.t + b * (size_t)(D.K * 256));
    atomicOr(&bad_all, bad); // the per-key verdict: an OR over the workgroup, whatever the data
    __syncthreads();
    store_block(D, L, tid, 256, bad_all, sk + D.pvb, a.se + b * a.se_stride, a.pk + b * a.pk_stride, a.ok + b);
}

bool witness_args_ok(const WitnessArgs &a)
{
    auto al = [](const void *p, size_t m) { return (reinterpret_cast<uintptr_t>(p) & (m - 1)) == 0; };
    // 16-byte copies of the embedded pk (offset 384 K, a multiple of 16) and 4-byte loads of s-hat: records on 16-byte boundaries;
    // 16-byte loads of A and t, 16-byte stores of s, e and the pk bytes
    return a.K >= 2 && a.K <= 4 && a.sk && a.A && a.t && a.se && a.pk && a.ok && al(a.sk, 16) && a.sk_stride % 16 == 0 && al(a.A, 16) && (a.A_stride * 2) % 16 == 0 &&
           al(a.t, 16) && al(a.se, 16) && (a.se_stride * 2) % 16 == 0 && al(a.pk, 16) && a.pk_stride % 16 == 0;
}

hipError_t launch_witness_from_sk(const WitnessArgs &a, int n, hipStream_t st)
{
    k_witness_from_sk<<<dim3((unsigned)n), dim3(256), 0, st>>>(a);
    return hipGetLastError();
}

} // namespace kosk
