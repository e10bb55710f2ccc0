// Fiat-Shamir aggregation on the GPU (round 6): the two 343-permutation chains per proof and role
//
//   h1 = sha3_256(Tcomm[0..1454))  -> alpha = BE16(SHAKE256-PRF(h1, 1)) % q          mlwe_prover.cpp:130-153, mlwe_verifier.cpp:37-65
//   ch = sha3_256(ch_seeds[0..1454)) -> I = opened set ("+inc, rescan" probing)       mlwe_prover.cpp:445-474, mlwe_verifier.cpp:634-683
//
// hashed where the commitment kernels wrote the tables, in HBM: nothing but 32 + 300 bytes per proof would have to reach the host,
// and with the challenge vectors / opened lists consumed on the device nothing does -- the four 46.5 KB-per-proof device-to-host
// copies of a step, the host's four hashing rounds and the four host round trips disappear.
// One wave per proof; the sponge is csrc/kosk_keccak_wave_dev.hpp (one state per wave, a word per lane).
//   k_fs_chain<FS_DIGEST>  sha3_256 of n long messages (kernel-level entry point kosk_sha3_256_batch_wave; tests, bench)
//   k_fs_chain<FS_ALPHA>   the challenge vector of every proof, [n][80] u16
//   k_fs_chain<FS_OPENED>  prover: I, its ascending complement, the window boundaries and the sorted opened list (what
//                          fs_opened_batch of kosk_host.cpp writes into a row of the opened-list table)
//   k_fs_chain<FS_CHECK>   verifier: I' recomputed and compared with the proof's own list, fail bit FB_OPENED_SET
// kyber/fips202.c:461-485, :723-734 (shake256), :745-754 (sha3_256); kyber/symmetric-shake.c:41-51 (kyber_shake256_prf).
#include <hip/hip_runtime.h>

#include "kosk_device.hpp"
#include "kosk_keccak_wave_dev.hpp"

namespace kosk {

namespace {

constexpr int FS_PF = 4; // message blocks in flight per wave (8 bytes per lane each)

__device__ __forceinline__ uint2 fs_load_word(const uint8_t *p)
{
    return *reinterpret_cast<const uint2 *>(p);
}

// the last (partial) block's word at byte offset 8 w of the remaining `rem` bytes, padded for the 136-byte rate
__device__ __forceinline__ uint2 fs_last_word(const uint8_t *tail, int rem, int w, uint32_t dom)
{
    uint32_t lo = 0, hi = 0;
    const int o = 8 * w;
    if (o + 8 <= rem) {
        const uint2 v = fs_load_word(tail + o);
        lo = v.x; hi = v.y;
    } else if (o < rem) {
        for (int i = 0; i < rem - o; i++) {
            const uint32_t byte = tail[o + i];
            if (i < 4) lo |= byte << (8 * i);
            else hi |= byte << (8 * (i - 4));
        }
    }
    const uint2 p = WaveSponge::pad(w, rem, dom, 136);
    return make_uint2(lo ^ p.x, hi ^ p.y);
}

// BOUND (kosk-bind-v1): the 32-byte binding value of the proof follows the table in the hashed message.  The table's
// tail is a whole number of words (1454 x 32 = 342 x 136 + 16: two words) and tail + 32 bytes stay inside the last block, so the
// chain has the same number of permutations as the unbound one: the last block's words are the tail's, then four of B, then the padding
// FORCED (tests, kosk_force_opened_candidates; FS_OPENED only): proofs b < A.cand_n read their 150 candidates from A.cand in place of the
// squeezed bytes; everything else is the same code, and the instantiations without it are what they were
template <int MODE, bool BOUND = false, bool FORCED = false>
__global__ __launch_bounds__(64) void k_fs_chain(FsArgs A)
{
    __shared__ __align__(16) uint32_t st[64];       // the state's words, to be re-interleaved by other lanes
    __shared__ __align__(16) uint8_t sq[3 * 136];   // squeezed PRF bytes
    __shared__ uint16_t pos[MODE >= FS_OPENED ? NPARTY : 1];
    __shared__ uint16_t il[MODE >= FS_OPENED ? NOPEN + 2 : 1];

    const int lane = threadIdx.x, b = blockIdx.x;
    __builtin_amdgcn_s_setprio(3); // a chain is latency, not throughput: its wave issues first wherever it shares a SIMD
    WaveSponge sp;
    sp.setup(lane);
    const int word = sp.word();

    // ---- sha3_256 of the table
    const uint8_t *src = A.in + (size_t)b * A.in_stride;
    const int nfull = A.len / 136, rem = A.len - nfull * 136;
    const bool ld = word < 17;
    const uint8_t *mine = src + 8 * (ld ? word : 0);
    uint32_t a = 0;
    uint2 pf[FS_PF];
#pragma unroll
    for (int j = 0; j < FS_PF; j++) pf[j] = (ld && j < nfull) ? fs_load_word(mine + (size_t)136 * j) : make_uint2(0, 0);
    for (int blk = 0; blk < nfull; blk += FS_PF) {
#pragma unroll
        for (int j = 0; j < FS_PF; j++) {
            if (blk + j < nfull) { // (uniform)
                const uint2 m = pf[j];
                const int nb = blk + j + FS_PF;
                pf[j] = (ld && nb < nfull) ? fs_load_word(mine + (size_t)136 * nb) : make_uint2(0, 0);
                sp.absorb(a, m); // (lanes beyond word 16 loaded zeros)
                sp.permute(a);
            }
        }
    }
    if constexpr (BOUND) {
        uint2 m = make_uint2(0, 0);
        if (ld) {
            const int tw = rem >> 3; // (launch_fs_chain: rem is a multiple of 8 and rem + 32 < 136)
            if (word < tw) m = fs_load_word(src + (size_t)136 * nfull + 8 * word);
            else if (word < tw + 4) m = fs_load_word(A.bind + (size_t)b * 32 + 8 * (word - tw));
            const uint2 p = WaveSponge::pad(word, rem + 32, 0x06u, 136);
            m.x ^= p.x; m.y ^= p.y;
        }
        sp.absorb(a, m);
    } else {
        sp.absorb(a, ld ? fs_last_word(src + (size_t)136 * nfull, rem, word, 0x06u) : make_uint2(0, 0));
    }
    sp.permute(a);
    if (A.out_digest) {
        const uint2 w = sp.words(a, st, 4);
        if (lane < 4) *reinterpret_cast<uint2 *>(A.out_digest + (size_t)b * 32 + 8 * lane) = w;
    }
    if constexpr (MODE == FS_DIGEST) return;

    // ---- SHAKE256-PRF(digest, nonce 1): the digest's words are the new block's words 0..3 as they stand (still interleaved)
    {
        uint2 m = WaveSponge::pad(word, 33, 0x1Fu, 136); // 33 bytes absorbed, SHAKE domain
        if (word == 4) m.x |= 0x01u;                     // byte 32: the nonce
        a = word < 4 ? a : 0u;
        sp.absorb(a, m);
    }
    constexpr int NSQ = MODE == FS_ALPHA ? 2 : 3;
#pragma unroll 1
    for (int s = 0; s < NSQ; s++) {
        sp.permute(a);
        const uint2 w = sp.words(a, st, 17);
        if (lane < 17) *reinterpret_cast<uint2 *>(sq + 136 * s + 8 * lane) = w;
    }
    wave_lds_handoff();

    if constexpr (MODE == FS_ALPHA) {
        // alpha_i = BE16 % q, i < J (mlwe_prover.cpp:137-142); the entries behind J stay zero
        for (int i = lane; i < 80; i += 64) {
            const uint32_t v = i < A.J ? (((uint32_t)sq[2 * i] << 8) | sq[2 * i + 1]) % (uint32_t)Q : 0u;
            A.alpha[(size_t)b * A.alpha_stride + i] = (uint16_t)v;
        }
        return;
    } else {
        // ---- the opened set: candidate BE16 % N, then the reference's "+inc, rescan" probing = the first free party at or behind
        // the candidate, cyclically, in list order (mlwe_prover.cpp:459-474; kosk_host.cpp opened_from_ch)
        uint32_t c[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int i = lane + 64 * k;
            c[k] = i < NOPEN ? (((uint32_t)sq[2 * i] << 8) | sq[2 * i + 1]) % (uint32_t)NPARTY : 0u;
            if constexpr (FORCED) {
                if (b < A.cand_n && i < NOPEN) c[k] = A.cand[(size_t)b * NOPEN + i]; // (launch_fs_chain's callers: every entry < NPARTY)
            }
        }
        for (int p = lane; p < NPARTY; p += 64) pos[p] = 0xFFFF;
        wave_lds_handoff();
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const int cnt = k < 2 ? 64 : NOPEN - 128;
            for (int j = 0; j < cnt; j++) {
                uint32_t v = (uint32_t)__builtin_amdgcn_readlane((int)c[k], j);
                while ((uint32_t)__builtin_amdgcn_readfirstlane((int)pos[v]) != 0xFFFFu) v = v + 1 == (uint32_t)NPARTY ? 0u : v + 1;
                if (lane == 0) {
                    pos[v] = (uint16_t)(64 * k + j);
                    il[64 * k + j] = (uint16_t)v;
                }
                wave_lds_handoff();
            }
        }
        if constexpr (MODE == FS_CHECK) {
            // I' == I of the proof image (mlwe_verifier.cpp:678-683)
            const uint16_t *given = reinterpret_cast<const uint16_t *>(A.proof + (size_t)b * A.image_stride + A.off_I);
            bool bad = false;
            for (int i = lane; i < NOPEN; i += 64) bad |= il[i] != given[i];
            if (__builtin_amdgcn_ballot_w64(bad) != 0 && lane == 0) atomicOr(A.fail + b, 1u << FB_OPENED_SET);
            return;
        } else {
            uint16_t *Ib = A.I + (size_t)b * A.sel_stride, *rb = A.rest + (size_t)b * A.sel_stride;
            for (int i = lane; i < NOPEN; i += 64) Ib[i] = il[i];
            // the ascending complement, the number of unopened parties below every multiple of 64 (window boundaries), and the opened
            // parties ascending with their positions in I (kosk_params.hpp: SEL_WIN, SEL_OSORT, SEL_OPOS)
            uint32_t nrest = 0, nopen = 0;
            for (int w = 0; w < NWIN; w++) {
                const int p = 64 * w + lane;
                const uint32_t at = p < NPARTY ? pos[p] : 0u;
                const bool in = p < NPARTY, opened = in && at != 0xFFFFu, closed = in && !opened;
                const uint64_t mo = __builtin_amdgcn_ballot_w64(opened), mc = __builtin_amdgcn_ballot_w64(closed);
                const uint64_t below = ((uint64_t)1 << lane) - 1;
                if (lane == 0) Ib[SEL_WIN + w] = (uint16_t)nrest;
                if (closed) rb[nrest + __popcll(mc & below)] = (uint16_t)p;
                if (opened) {
                    const uint32_t k = nopen + __popcll(mo & below);
                    Ib[SEL_OSORT + k] = (uint16_t)p;
                    Ib[SEL_OPOS + k] = (uint16_t)at;
                }
                nrest += __popcll(mc);
                nopen += __popcll(mo);
            }
            if (lane == 0) Ib[SEL_WIN + NWIN] = (uint16_t)nrest;
        }
    }
}

// B = sha3_256("kosk-bind-v1" || 00 00 00 00 || LE32(K) || sha3_256(pk) || context), 84 bytes, for proof b = blockIdx.x.  One wave per
// proof on the wave sponge: 6 / 9 / 12 permutations for the public key and one for the outer message, a 27th of a chain, and as
// parallel as the chains that wait for it.  pk and contexts: bases and pk_stride multiples of 8 (launch_bind_values)
__global__ __launch_bounds__(64) void k_bind_values(BindArgs A)
{
    __shared__ __align__(16) uint32_t st[64];
    __shared__ __align__(16) uint32_t msg[34]; // the outer message's only block
    const int lane = threadIdx.x, b = blockIdx.x;
    WaveSponge sp;
    sp.setup(lane);
    const int word = sp.word();
    const bool ld = word < 17;

    const uint8_t *src = A.pk + (size_t)b * A.pk_stride;
    const int nfull = A.pk_bytes / 136, rem = A.pk_bytes - nfull * 136;
    const uint8_t *mine = src + 8 * (ld ? word : 0);
    uint32_t a = 0;
    uint2 nx = (ld && nfull > 0) ? fs_load_word(mine) : make_uint2(0, 0);
#pragma unroll 1
    for (int blk = 0; blk < nfull; blk++) {
        const uint2 m = nx;
        nx = (ld && blk + 1 < nfull) ? fs_load_word(mine + (size_t)136 * (blk + 1)) : make_uint2(0, 0);
        sp.absorb(a, m);
        sp.permute(a);
    }
    sp.absorb(a, ld ? fs_last_word(src + (size_t)136 * nfull, rem, word, 0x06u) : make_uint2(0, 0));
    sp.permute(a);
    const uint2 hw = sp.words(a, st, 4); // sha3_256(pk): bytes 20..51 of the outer message

    if (lane < 4) { msg[5 + 2 * lane] = hw.x; msg[6 + 2 * lane] = hw.y; }
    if (lane < 8) msg[13 + lane] = *reinterpret_cast<const uint32_t *>(A.contexts + (size_t)b * 32 + 4 * lane); // bytes 52..83
    if (lane >= 8 && lane < 21) msg[13 + lane] = lane == 8 ? 0x06u : lane == 20 ? 0x80000000u : 0u; // padding: byte 84, byte 135
    if (lane >= 21 && lane < 26) {
        constexpr uint32_t head[5] = {0x6b736f6bu, 0x6e69622du, 0x31762d64u, 0u, 0u}; // "kosk-bind-v1", four zero bytes, then K
        msg[lane - 21] = lane == 25 ? (uint32_t)A.K : head[lane - 21];
    }
    wave_lds_handoff();
    a = 0;
    sp.absorb(a, ld ? make_uint2(msg[2 * word], msg[2 * word + 1]) : make_uint2(0, 0));
    sp.permute(a);
    const uint2 w = sp.words(a, st, 4);
    if (lane < 4) *reinterpret_cast<uint2 *>(A.out + (size_t)b * 32 + 8 * lane) = w;
}

// kosk-keyseed-v1: seed_b = SHAKE256("kosk-keyseed-v1" || 00 || LE32(K) || LE32(flags) || context[32] || salt[32] || sk_b)[0:32],
// one wave per key on the wave sponge, 13 / 19 / 24 permutations for K = 2 / 3 / 4.  Word g = 17 blk + w of the message is word g of
// the 11-word header for g < 11 (all of it in block 0, built in registers) and word g - 11 of the sk record behind it; the record is a
// whole number of words, so is the last block (88 / 40 / 128 bytes).  sk, salt and seed are secret: every address and every branch is
// a function of K, the flags, blk and the lane alone.  Bases and strides multiples of 8 (launch_keyseed)
__global__ __launch_bounds__(64) void k_keyseed(KeyseedArgs A)
{
    __shared__ __align__(16) uint32_t st[64];
    const int lane = threadIdx.x, b = blockIdx.x;
    WaveSponge sp;
    sp.setup(lane);
    const int word = sp.word();
    const bool ld = word < 17;

    const uint8_t *sk = A.sk + (size_t)b * A.sk_stride;
    const int len = 88 + A.sk_bytes, nfull = len / 136, rem = len - nfull * 136; // (launch_keyseed: nfull >= 1, rem % 8 == 0)
    const uint32_t flags = (A.contexts ? 1u : 0u) | (A.salts ? 2u : 0u);
    // block 0: the header's words, then the record's first six
    uint2 nx = make_uint2(0, 0);
    if (word == 0) nx = make_uint2(0x6b736f6bu, 0x79656b2du);      // "kosk-key"
    else if (word == 1) nx = make_uint2(0x64656573u, 0x0031762du); // "seed-v1", 00
    else if (word == 2) nx = make_uint2((uint32_t)A.K, flags);
    else if (word < 7) { if (A.contexts) nx = fs_load_word(A.contexts + (size_t)b * A.context_stride + 8 * (word - 3)); }
    else if (word < 11) { if (A.salts) nx = fs_load_word(A.salts + (size_t)b * A.salt_stride + 8 * (word - 7)); }
    else if (ld) nx = fs_load_word(sk + 8 * (word - 11));
    const size_t mine = 8 * (size_t)(ld ? word : 0); // word w of block blk >= 1: byte 136 blk - 88 + 8 w of the record
    uint32_t a = 0;
#pragma unroll 1
    for (int blk = 0; blk < nfull; blk++) {
        const uint2 m = nx;
        // the next block's word is in flight under this block's permutation; the last block brings the padding (uniform branch)
        if (blk + 1 < nfull) nx = ld ? fs_load_word(sk + ((size_t)136 * (blk + 1) - 88 + mine)) : make_uint2(0, 0);
        else nx = ld ? fs_last_word(sk + (size_t)136 * nfull - 88, rem, word, 0x1Fu) : make_uint2(0, 0);
        sp.absorb(a, m);
        sp.permute(a);
    }
    sp.absorb(a, nx);
    sp.permute(a);
    const uint2 w = sp.words(a, st, 4);
    if (lane < 4) *reinterpret_cast<uint2 *>(A.out + (size_t)b * 32 + 8 * lane) = w;
}

} // namespace

hipError_t launch_bind_values(const BindArgs &A, int n, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    auto misaligned = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7) != 0; };
    if (!A.pk || !A.contexts || !A.out || A.pk_bytes < 8 || A.pk_bytes % 8 || A.pk_stride % 8 || A.pk_stride < (size_t)A.pk_bytes ||
        misaligned(A.pk) || misaligned(A.contexts) || misaligned(A.out)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bind_values, dim3(n), dim3(64), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_keyseed(const KeyseedArgs &A, int n, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    auto misaligned = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 7) != 0; };
    if (!A.sk || !A.out || A.K < 2 || A.K > 4 || A.sk_bytes != 768 * A.K + 96 || A.sk_stride % 8 || A.sk_stride < (size_t)A.sk_bytes || misaligned(A.sk) ||
        misaligned(A.out) || (A.contexts && (misaligned(A.contexts) || A.context_stride % 8 || A.context_stride < 32)) ||
        (A.salts && (misaligned(A.salts) || A.salt_stride % 8 || A.salt_stride < 32))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_keyseed, dim3(n), dim3(64), 0, st, A);
    return hipGetLastError();
}

hipError_t launch_fs_chain(const FsArgs &A, int mode, int n, hipStream_t st)
{
    if (n <= 0) return hipSuccess;
    if (mode < FS_DIGEST || mode > FS_CHECK) return hipErrorInvalidValue;
    const bool forced = A.cand && A.cand_n > 0;
    if (forced && mode != FS_OPENED) return hipErrorInvalidValue;
    if (A.bind) { // kosk-bind-v1: the bound instantiations (the unbound ones below are what they were)
        const int rem = A.len % 136;
        if (mode == FS_DIGEST || rem % 8 || rem + 32 >= 136 || (reinterpret_cast<uintptr_t>(A.bind) & 7)) return hipErrorInvalidValue;
        switch (mode) {
        case FS_ALPHA: hipLaunchKernelGGL((k_fs_chain<FS_ALPHA, true>), dim3(n), dim3(64), 0, st, A); break;
        case FS_OPENED:
            if (forced) hipLaunchKernelGGL((k_fs_chain<FS_OPENED, true, true>), dim3(n), dim3(64), 0, st, A);
            else hipLaunchKernelGGL((k_fs_chain<FS_OPENED, true>), dim3(n), dim3(64), 0, st, A);
            break;
        default: hipLaunchKernelGGL((k_fs_chain<FS_CHECK, true>), dim3(n), dim3(64), 0, st, A); break;
        }
        return hipGetLastError();
    }
    switch (mode) {
    case FS_DIGEST: hipLaunchKernelGGL(k_fs_chain<FS_DIGEST>, dim3(n), dim3(64), 0, st, A); break;
    case FS_ALPHA: hipLaunchKernelGGL(k_fs_chain<FS_ALPHA>, dim3(n), dim3(64), 0, st, A); break;
    case FS_OPENED:
        if (forced) hipLaunchKernelGGL((k_fs_chain<FS_OPENED, false, true>), dim3(n), dim3(64), 0, st, A);
        else hipLaunchKernelGGL(k_fs_chain<FS_OPENED>, dim3(n), dim3(64), 0, st, A);
        break;
    default: hipLaunchKernelGGL(k_fs_chain<FS_CHECK>, dim3(n), dim3(64), 0, st, A); break;
    }
    return hipGetLastError();
}

} // namespace kosk
