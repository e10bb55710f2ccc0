// The handoff of LDS data between the lanes of ONE wave (a single-wave workgroup, or an LDS area only one wave touches).
#pragma once
#include <hip/hip_runtime.h>

namespace kosk {

// Put between the LDS stores of some lanes and the LDS loads (or overwriting stores) of others.  The hardware needs nothing here: one
// wave's LDS operations execute in issue order, so a store is visible to every load issued behind it.  The fences are for the
// COMPILER: __builtin_amdgcn_wave_barrier() is declared without memory effects -- a scheduling barrier, not a fence -- and alone it
// would let an access be moved or forwarded across the handoff wherever alias analysis allows.  Release before and acquire after, at
// wavefront scope, forbid that and emit no instruction.  Data that arrives by global loads still needs its s_waitcnt in front.
__device__ __forceinline__ void wave_lds_handoff()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

} // namespace kosk
