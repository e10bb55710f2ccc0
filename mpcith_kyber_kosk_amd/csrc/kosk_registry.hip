// The verified-key registry: a table of admitted Kyber public keys in HBM.  What depends on a key alone --
// the pk bytes, H(pk), A^T: 36 of the 37 Keccak permutations of a Kyber-768 encapsulation -- is computed once, at admission, by
// k_registry_admit; kem_enc_slots (kosk_kem_kernels.hip) then runs the per-item kernels with the registry as their key side, item b's key
// pieces at base + slot[b] * stride.
//
//   admission   k_registry_admit   per accepted key: the K^2 entries of A^T straight into the slot, H(pk), the pk bytes in 16-byte stores, the flag
//     up to KEM_WAVE_MAX keys      K^2 + 1 one-wave blocks per key (the shape of k_kem_key_setup for n keys): one matrix entry on lane 0 of a
//                                  block, the entries side by side; H(pk) on the wave sponge, whose block then copies the bytes
//     above                        one sponge per lane in task-major lane ranges, longest role first (as k_kem_hash): H(pk), then the K^2
//                                  entries; the copy is a flat range behind them, consecutive lanes on consecutive 16-byte lines of one key
//   eviction    k_wipe             the slots' four pieces are regions of a wipe
//   index       k_registry_index   one lane per slot: open addressing over the slots' H(pk), rebuilt whole by the first lookup after a mutation
//   lookup      k_registry_find    one lane per query: the slot (or -1), or the slot index and mask the per-item KEM kernels read
//   tree        k_registry_tree    one block per 1 024 inputs of a tier: up to 10 levels of kosk-regtree-v1 through LDS, every node to HBM
//   paths       k_registry_path    one lane per 16-byte half of a sibling record
// slot[b] and the accept bit (slot[b] < 0: masked, nothing is written) are public; the admission reads nothing secret.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "kosk_ctx.hpp"
#include "kosk_keccak_wave_dev.hpp"
#include "kosk_kem_dev.hpp"
#include "kosk_regtree.hpp"

namespace kosk {

using namespace kem;

#define HIPCHK(x) KOSK_HIPCHK(x)

// A^T[i][j] = XOF(rho, i, j) (indcpa.c:177-178) of entry t = i K + j, as the matrix role of k_kem_hash
__device__ __forceinline__ void registry_entry(const RegAdmitJob &j, const uint8_t *src, size_t s, int t)
{
    uint64_t rho[4];
#pragma unroll
    for (int l = 0; l < 4; l++) rho[l] = ld64(src + j.pk_bytes - 32, l);
    if (!matrix_entry(rho, t / j.K, t % j.K, j.max_blocks, j.A + (s * (size_t)(j.K * j.K) + t) * 256))
        if (j.err) *reinterpret_cast<volatile uint32_t *>(j.err) = DEVERR_XOF_BLOCKS;
}

__global__ __launch_bounds__(64) void k_registry_admit(RegAdmitJob j)
{
    __shared__ __align__(16) uint32_t st[64];
    const int lane = threadIdx.x, KK = j.K * j.K, lines = j.pk_bytes / 16;
    if (j.wave) { // block t n + b: task t of key b (block-uniform)
        const int t = (int)(blockIdx.x / (unsigned)j.n), b = (int)(blockIdx.x - (unsigned)t * (unsigned)j.n);
        const int slot = j.slot[b];
        if (slot < 0) return;
        const uint8_t *src = j.src + (size_t)b * j.src_stride;
        if (t < KK) {
            if (lane == 0) registry_entry(j, src, (size_t)slot, t);
            return;
        }
        __builtin_amdgcn_s_setprio(3); // a chain is latency, not throughput
        WaveSponge sp;
        sp.setup(lane);
        uint32_t a = 0;
        wave_absorb_words(sp, a, [&](int i) { return *reinterpret_cast<const uint2 *>(src + 8 * i); }, j.pk_bytes / 8, 0x06u);
        const uint2 w = sp.words(a, st, 4);
        if (lane < 4) *reinterpret_cast<uint2 *>(j.h + (size_t)slot * 32 + 8 * lane) = w;
        const U128 *in = reinterpret_cast<const U128 *>(src);
        U128 *out = reinterpret_cast<U128 *>(j.pk + (size_t)slot * j.pk_bytes);
        for (int i = lane; i < lines; i += 64) out[i] = in[i];
        if (lane == 0) j.flag[slot] = 1;
        return;
    }
    const long gid = (long)blockIdx.x * 64 + lane, sponges = (long)(1 + KK) * j.n;
    if (gid < sponges) { // lane t n + b: H(pk) (t = 0: 6 / 9 / 12 permutations), then entry t - 1 (three or four)
        const int t = (int)(gid / j.n), b = (int)(gid - (long)t * j.n);
        const int slot = j.slot[b];
        if (slot < 0) return;
        const uint8_t *src = j.src + (size_t)b * j.src_stride;
        if (t) { registry_entry(j, src, (size_t)slot, t - 1); return; }
        uint64_t d[4];
        sha3_256_words(src, j.pk_bytes, d);
        U128 *o = reinterpret_cast<U128 *>(j.h + (size_t)slot * 32);
        o[0] = U128{(uint32_t)d[0], (uint32_t)(d[0] >> 32), (uint32_t)d[1], (uint32_t)(d[1] >> 32)};
        o[1] = U128{(uint32_t)d[2], (uint32_t)(d[2] >> 32), (uint32_t)d[3], (uint32_t)(d[3] >> 32)};
        j.flag[slot] = 1;
        return;
    }
    const long c = gid - sponges; // line c % lines of key c / lines
    if (c >= (long)lines * j.n) return;
    const int b = (int)(c / lines), i = (int)(c - (long)b * lines);
    const int slot = j.slot[b];
    if (slot < 0) return;
    reinterpret_cast<U128 *>(j.pk + (size_t)slot * j.pk_bytes)[i] = reinterpret_cast<const U128 *>(j.src + (size_t)b * j.src_stride)[i];
}

hipError_t launch_registry_admit(const RegAdmitJob &j, hipStream_t st)
{
    const long KK = (long)j.K * j.K;
    const long blocks = j.wave ? (KK + 1) * j.n : (((KK + 1) + j.pk_bytes / 16) * j.n + 63) / 64;
    k_registry_admit<<<dim3((unsigned)blocks), dim3(64), 0, st>>>(j);
    return hipGetLastError();
}

// ---- the fingerprint index ------------------------------------------------------------------------------
// T int32 entries, -1 = empty; the home of a fingerprint is LE32(h[0..4)) & (T - 1), probing is linear.  Fingerprints and slots are public:
// branches and addresses may depend on them.
__device__ __forceinline__ bool same_fingerprint(const U128 &a0, const U128 &a1, const uint8_t *p)
{
    const U128 b0 = reinterpret_cast<const U128 *>(p)[0], b1 = reinterpret_cast<const U128 *>(p)[1];
    return ((a0.x ^ b0.x) | (a0.y ^ b0.y) | (a0.z ^ b0.z) | (a0.w ^ b0.w) | (a1.x ^ b1.x) | (a1.y ^ b1.y) | (a1.z ^ b1.z) | (a1.w ^ b1.w)) == 0;
}

// One lane per slot.  An occupied slot s claims the first empty entry of its walk, or joins the entry that already belongs to its fingerprint
// (atomicMin: the lowest slot stays).  An entry never changes its fingerprint class once claimed, so what a lookup returns does not depend on
// the order of arrival, though entry positions may.  Every access to an entry is an atomic at agent scope (the table is shared across XCDs)
// and the atomics' return values are the only reads of entries.  The walk ends after T steps at the latest.
__global__ __launch_bounds__(256) void k_registry_index(RegIndexJob j)
{
    const long s = (long)blockIdx.x * 256 + threadIdx.x;
    if (s >= j.capacity || !j.flag[s]) return;
    const U128 h0 = reinterpret_cast<const U128 *>(j.h + (size_t)s * 32)[0], h1 = reinterpret_cast<const U128 *>(j.h + (size_t)s * 32)[1];
    uint32_t e = h0.x & j.mask;
    for (uint64_t step = 0; step <= j.mask; step++, e = (e + 1) & j.mask) {
        int32_t o = -1; // expected; the value found on failure
        if (__hip_atomic_compare_exchange_strong(j.index + e, &o, (int32_t)s, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) return;
        if (o < 0 || o >= j.capacity) break; // no slot number: never written by this kernel
        if (same_fingerprint(h0, h1, j.h + (size_t)o * 32)) {
            (void)__hip_atomic_fetch_min(j.index + e, (int32_t)s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            return;
        }
    }
    if (j.err) *reinterpret_cast<volatile uint32_t *>(j.err) = DEVERR_INDEX_FULL;
}

// One lane per query: from the home to the first empty entry (a miss) or the first entry whose slot holds the query's fingerprint (a hit),
// T steps at the latest.  A miss writes key 0, not -1: the seed role of k_kem_hash reads h at key[b] before it looks at the mask
__global__ __launch_bounds__(64) void k_registry_find(RegFindJob j)
{
    const long b = (long)blockIdx.x * 64 + threadIdx.x;
    if (b >= j.n) return;
    const U128 q0 = reinterpret_cast<const U128 *>(j.q + (size_t)b * 32)[0], q1 = reinterpret_cast<const U128 *>(j.q + (size_t)b * 32)[1];
    uint32_t e = q0.x & j.mask;
    int32_t hit = -1;
    bool ended = false;
    for (uint64_t step = 0; step <= j.mask; step++, e = (e + 1) & j.mask) {
        const int32_t o = j.index[e];
        if (o < 0 || o >= j.capacity) { ended = true; break; } // empty (k_registry_index writes nothing but -1 and slot numbers)
        if (same_fingerprint(q0, q1, j.h + (size_t)o * 32)) { hit = o; ended = true; break; }
    }
    if (!ended && j.err) *reinterpret_cast<volatile uint32_t *>(j.err) = DEVERR_INDEX_FULL;
    if (j.slot) j.slot[b] = hit;
    if (j.key) {
        j.key[b] = hit < 0 ? 0 : hit;
        j.found[b] = hit >= 0;
    }
}

hipError_t launch_registry_index(const RegIndexJob &j, hipStream_t st)
{
    k_registry_index<<<dim3((unsigned)((j.capacity + 255) / 256)), dim3(256), 0, st>>>(j);
    return hipGetLastError();
}

hipError_t launch_registry_find(const RegFindJob &j, hipStream_t st)
{
    k_registry_find<<<dim3((unsigned)((j.n + 63) / 64)), dim3(64), 0, st>>>(j);
    return hipGetLastError();
}

// ---- the registry tree (kosk-regtree-v1, kosk_regtree.hpp) -------------------------------------------------
// Every hash is ONE permutation: the inputs are 20, 52 and 80 bytes of a 136-byte rate block, so a lane builds the padded block in its state
// and permutes once (the one-state-per-lane Keccak of kosk_keccak_dev.hpp).  Fingerprints, flags and slot numbers are public.
__device__ __forceinline__ void regtree_store(uint8_t *dst, const uint64_t (&d)[4])
{
    U128 *o = reinterpret_cast<U128 *>(dst);
    o[0] = U128{(uint32_t)d[0], (uint32_t)(d[0] >> 32), (uint32_t)d[1], (uint32_t)(d[1] >> 32)};
    o[1] = U128{(uint32_t)d[2], (uint32_t)(d[2] >> 32), (uint32_t)d[3], (uint32_t)(d[3] >> 32)};
}
__device__ __forceinline__ void regtree_load(const uint8_t *src, uint64_t (&d)[4])
{
    const U128 a = reinterpret_cast<const U128 *>(src)[0], b = reinterpret_cast<const U128 *>(src)[1];
    d[0] = (uint64_t)a.x | (uint64_t)a.y << 32; d[1] = (uint64_t)a.z | (uint64_t)a.w << 32;
    d[2] = (uint64_t)b.x | (uint64_t)b.y << 32; d[3] = (uint64_t)b.z | (uint64_t)b.w << 32;
}

// One block, one subtree of a tier: `cnt` <= 1 024 inputs, then `up` <= 10 levels, level by level through LDS (two buffers, 32 KB + 16 KB,
// a barrier between levels); every node also goes to its place in the level-major tree.  Block q of an upper tier owns nodes
// [q (1024 >> lv), (q + 1) (1024 >> lv)) of level 10 tier + lv.  All loop bounds are block-uniform.
__global__ __launch_bounds__(256) void k_registry_tree(RegTreeJob j)
{
    __shared__ __align__(16) uint64_t lds[(regtree::TIER_INPUTS + regtree::TIER_INPUTS / 2) * 4];
    const int tid = threadIdx.x, L0 = j.tier * regtree::TIER_LEVELS;
    const size_t q = j.tier ? (size_t)blockIdx.x : (size_t)j.list[blockIdx.x];
    const int cnt = j.D - L0 >= regtree::TIER_LEVELS ? (int)regtree::TIER_INPUTS : 1 << (j.D - L0);
    const int up = j.D - L0 >= regtree::TIER_LEVELS ? (int)regtree::TIER_LEVELS : j.D - L0;
    uint8_t *in_lvl = j.tree + regtree::level_offset(j.D, L0) + q * regtree::TIER_INPUTS * 32;
    for (int i = tid; i < cnt; i += 256) {
        uint64_t d[4];
        if (j.tier) {
            regtree_load(in_lvl + (size_t)i * 32, d);
        } else {
            const size_t s = q * regtree::TIER_INPUTS + (size_t)i;
            if (s < (size_t)j.capacity && j.flag[s]) {
                uint64_t h[4], st[25];
                regtree_load(j.h + s * 32, h);
                regtree::leaf_state(st, j.K, h);
                perm(st);
#pragma unroll
                for (int l = 0; l < 4; l++) d[l] = st[l];
            } else {
#pragma unroll
                for (int l = 0; l < 4; l++) d[l] = j.empty[l];
            }
            regtree_store(in_lvl + (size_t)i * 32, d);
        }
#pragma unroll
        for (int l = 0; l < 4; l++) lds[4 * i + l] = d[l];
    }
    __syncthreads();
    int in = 0, out = regtree::TIER_INPUTS * 4; // word offsets of the two buffers
    int lv = 1;
    for (; lv <= up && (cnt >> lv) > j.wave_tail; lv++) { // one sponge per lane
        const int m = cnt >> lv;
        uint8_t *dst = j.tree + regtree::level_offset(j.D, L0 + lv) + q * (size_t)(regtree::TIER_INPUTS >> lv) * 32;
        for (int i = tid; i < m; i += 256) {
            uint64_t l[4], r[4], st[25];
#pragma unroll
            for (int w = 0; w < 4; w++) { l[w] = lds[in + 8 * i + w]; r[w] = lds[in + 8 * i + 4 + w]; }
            regtree::node_state(st, l, r);
            perm(st);
#pragma unroll
            for (int w = 0; w < 4; w++) { l[w] = st[w]; lds[out + 4 * i + w] = st[w]; }
            regtree_store(dst + (size_t)i * 32, l);
        }
        __syncthreads();
        const int t = in; in = out; out = t;
    }
    if (lv > up) return;
    // the last levels, wave_tail nodes or fewer: a chain of single permutations that would run on a nearly empty wave -- one WAVE per node on
    // the wave sponge instead, the block's four waves side by side (DESIGN.md 37 has the measurement that chose wave_tail)
    __shared__ __align__(16) uint32_t wst[4][64];
    const int wave = tid >> 6, lane = tid & 63;
    WaveSponge sp;
    sp.setup(lane);
    for (; lv <= up; lv++) {
        const int m = cnt >> lv;
        uint8_t *dst = j.tree + regtree::level_offset(j.D, L0 + lv) + q * (size_t)(regtree::TIER_INPUTS >> lv) * 32;
        for (int i = wave; i < m; i += 4) { // wave-uniform
            const uint64_t *src = lds + in + 8 * i;
            uint32_t a = 0;
            wave_absorb_words(sp, a, [&](int w) {
                const uint64_t v = w == 0 ? regtree::TAG0 : w == 1 ? (regtree::TAG1 | 2ULL << 56) : src[w - 2];
                return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
            }, 10, 0x06u);
            const uint2 d = sp.words(a, wst[wave], 4);
            if (lane < 4) {
                lds[out + 4 * i + lane] = (uint64_t)d.x | (uint64_t)d.y << 32;
                *reinterpret_cast<uint2 *>(dst + (size_t)i * 32 + 8 * lane) = d;
            }
        }
        __syncthreads();
        const int t = in; in = out; out = t;
    }
}

// One lane per 16-byte half of a record; records 0 .. D - 1 of an item are its path, record D carries the slot's fingerprint and the found bit
__global__ __launch_bounds__(256) void k_registry_path(RegPathJob j)
{
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const int per = 2 * (j.D + 1);
    if (gid >= (long)per * j.n) return;
    const long b = gid / per;
    const int r = (int)(gid - b * per), l = r >> 1, half = r & 1;
    const int32_t s = j.slot[b];
    U128 v{0, 0, 0, 0};
    if (l < j.D) {
        if (s >= 0) v = reinterpret_cast<const U128 *>(j.tree + regtree::level_offset(j.D, l) + (((size_t)s >> l) ^ 1) * 32)[half];
        reinterpret_cast<U128 *>(j.paths)[((size_t)b * j.D + l) * 2 + half] = v;
        return;
    }
    if (j.hout) {
        if (s >= 0) v = reinterpret_cast<const U128 *>(j.h + (size_t)s * 32)[half];
        reinterpret_cast<U128 *>(j.hout)[(size_t)b * 2 + half] = v;
    }
    if (j.found && !half) j.found[b] = s >= 0;
}

hipError_t launch_registry_tree(const RegTreeJob &j, unsigned blocks, hipStream_t st)
{
    k_registry_tree<<<dim3(blocks), dim3(256), 0, st>>>(j);
    return hipGetLastError();
}

hipError_t launch_registry_path(const RegPathJob &j, hipStream_t st)
{
    const long lanes = 2L * (j.D + 1) * j.n;
    k_registry_path<<<dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st>>>(j);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- host --
// KOSK_DEBUG_REGTREE_WAVE_TAIL=m moves the boundary between the two sponge layouts of k_registry_tree: levels of m nodes or fewer run on the
// wave sponge (0: none); read at every rebuild, so a measurement can alternate the settings in one process
static int regtree_wave_tail()
{
    const char *e = getenv("KOSK_DEBUG_REGTREE_WAVE_TAIL");
    const int v = e ? atoi(e) : (int)REGTREE_WAVE_TAIL;
    return v < 0 ? 0 : v > 64 ? 64 : v;
}

int registry_tree_ensure(Ctx &c, KemRegistry &r)
{
    if (r.tree_valid) return 0;
    HIPCHK(hipSetDevice(c.device));
    const int D = regtree::depth(r.capacity), S = regtree::subtrees(D), T = regtree::tiers(D);
    if (!r.d_tree) { // public, both: hashes of public fingerprints, subtree numbers
        const int G = r.inv_group;
        HIPCHK(c.own(r.buf_name("registry.d_dirty", "monitor.d_dirty"), &r.d_dirty, (size_t)S * sizeof(int32_t), 0, G));
        if (c.own(r.buf_name("registry.d_tree", "monitor.d_tree"), &r.d_tree, regtree::tree_bytes(r.capacity), 0, G) != hipSuccess) { // both or neither
            void **at = reinterpret_cast<void **>(&r.d_dirty);
            c.inv.release_if([at](const InvBuf &b) { return b.at == at; });
            (void)hipGetLastError();
            c.err = "registry_tree_ensure: out of memory for the tree";
            return -1;
        }
        r.dirty.assign((size_t)S, 1); // the first build hashes every leaf subtree
    }
    std::vector<int32_t> list;
    for (int q = 0; q < S; q++)
        if (r.dirty[(size_t)q]) list.push_back(q);
    RegTreeJob j{};
    j.D = D; j.K = c.P.K; j.capacity = r.capacity; j.h = r.d_h; j.flag = r.d_flag; j.list = r.d_dirty; j.tree = r.d_tree;
    j.wave_tail = regtree_wave_tail();
    uint8_t e[32];
    (void)regtree::leaf(c.P.K, nullptr, e);
    memcpy(j.empty, e, 32);
    if (!list.empty()) {
        HIPCHK(hipMemcpyAsync(r.d_dirty, list.data(), list.size() * sizeof(int32_t), hipMemcpyHostToDevice, c.stream));
        HIPCHK(launch_registry_tree(j, (unsigned)list.size(), c.stream));
        c.path_n[PATH_REGISTRY_TREE]++;
        c.path_n[PATH_REGISTRY_SUBTREES] += (long)list.size();
        for (int t = 1; t < T; t++) { // the upper tiers whole: at most P / 1024 + ... nodes
            j.tier = t;
            const int above = D - t * regtree::TIER_LEVELS;
            HIPCHK(launch_registry_tree(j, above > regtree::TIER_LEVELS ? 1u << (above - regtree::TIER_LEVELS) : 1u, c.stream));
            c.path_n[PATH_REGISTRY_TREE]++;
        }
        // paths staged from the earlier tree state go with it: after an eviction and this rebuild no hash of the evicted key is left
        if (r.d_paths) HIPCHK(hipMemsetAsync(r.d_paths, 0, r.paths_cap, c.stream));
        HIPCHK(stream_sync(c));
        std::fill(r.dirty.begin(), r.dirty.end(), 0);
    }
    r.tree_valid = true;
    return 0;
}

int registry_paths_ensure(Ctx &c, int n)
{
    KemRegistry &r = *c.registry;
    const size_t need = (size_t)((n + 1023) / 1024 * 1024) * regtree::depth(r.capacity) * 32;
    if (need <= r.paths_cap) return 0;
    HIPCHK(hipSetDevice(c.device));
    if (r.d_paths) {
        HIPCHK(stream_sync(c));
        void **at = reinterpret_cast<void **>(&r.d_paths);
        c.inv.release_if([at](const InvBuf &b) { return b.at == at; });
        r.paths_cap = 0;
    }
    HIPCHK(c.own("registry.d_paths", &r.d_paths, need, 0, Inventory::INVG_REGISTRY)); // public: copies of tree nodes
    r.paths_cap = need;
    return 0;
}

int registry_root(Ctx &c, KemRegistry &r, uint8_t *root)
{
    if (registry_tree_ensure(c, r)) return -1;
    const int D = regtree::depth(r.capacity);
    HIPCHK(hipMemcpyAsync(root, r.d_tree + regtree::level_offset(D, D), 32, is_device_pointer(root) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c.stream));
    HIPCHK(stream_sync(c));
    return 0;
}

int registry_index_ensure(Ctx &c)
{
    KemRegistry &r = *c.registry;
    if (r.index_valid) return 0;
    HIPCHK(hipSetDevice(c.device));
    const size_t T = registry_index_entries(r.capacity);
    if (!r.d_index) HIPCHK(c.own("registry.d_index", &r.d_index, T * sizeof(int32_t), 0, Inventory::INVG_REGISTRY)); // public: slot numbers only
    HIPCHK(hipMemsetAsync(r.d_index, 0xFF, T * sizeof(int32_t), c.stream));
    RegIndexJob j{};
    j.capacity = r.capacity; j.mask = (uint32_t)(T - 1); j.h = r.d_h; j.flag = r.d_flag; j.index = r.d_index; j.err = c.h_err;
    HIPCHK(launch_registry_index(j, c.stream));
    c.path_n[PATH_REGISTRY_INDEX]++;
    HIPCHK(stream_sync(c));
    if (device_error_check(c)) return -1; // index overflow
    r.index_valid = true;
    return 0;
}

void registry_release(Ctx &c)
{
    KemRegistry *r = c.registry;
    if (!r) return;
    headsig_signer_release(c); // the signer signs this registry's history
    c.inv.release(Inventory::INVG_REGISTRY);
    delete r;
    c.registry = nullptr;
}

int registry_reserve(Ctx &c, int capacity)
{
    if (capacity < 0) { c.err = "kosk_registry_reserve: capacity < 0"; return -1; }
    if (c.registry && c.registry->used) { c.err = "kosk_registry_reserve: the registry is not empty (kosk_registry_evict)"; return -1; }
    HIPCHK(hipSetDevice(c.device));
    if (c.registry) {
        HIPCHK(stream_sync(c));
        registry_release(c); // every slot is empty, and an empty slot is zeros
    }
    if (!capacity) return 0;
    const Dims D = dims(c.P.K);
    KemRegistry *r = new KemRegistry();
    c.registry = r;
    const size_t N = (size_t)capacity, a_bytes = N * D.K * D.K * 512;
    const int G = Inventory::INVG_REGISTRY; // public, all four: the wipes leave them alone, the scan covers them
    auto body = [&]() -> int {
        HIPCHK(c.own("registry.d_pk", &r->d_pk, N * D.pk, 0, G));
        HIPCHK(c.own("registry.d_h", &r->d_h, N * 32, 0, G));
        HIPCHK(c.own("registry.d_A", &r->d_A, a_bytes, 0, G));
        HIPCHK(c.own("registry.d_flag", &r->d_flag, N, 0, G));
        HIPCHK(hipMemsetAsync(r->d_pk, 0, N * D.pk, c.stream));
        HIPCHK(hipMemsetAsync(r->d_h, 0, N * 32, c.stream));
        HIPCHK(hipMemsetAsync(r->d_A, 0, a_bytes, c.stream));
        HIPCHK(hipMemsetAsync(r->d_flag, 0, N, c.stream));
        HIPCHK(stream_sync(c));
        return 0;
    };
    if (body()) {
        const std::string why = c.err;
        (void)hipGetLastError();
        registry_release(c); // nothing is left allocated
        c.err = "kosk_registry_reserve: " + why;
        return -1;
    }
    r->capacity = capacity;
    r->occ.assign(N, 0);
    return 0;
}

int registry_evict(Ctx &c, int n, const int32_t *slots)
{
    KemRegistry &r = *c.registry;
    const Dims D = dims(c.P.K);
    HIPCHK(hipSetDevice(c.device));
    r.lookups_stale();
    const size_t a_bytes = (size_t)D.K * D.K * 512;
    std::vector<WipeRegion> dev;
    for (int b = 0; b < n; b++) {
        const size_t s = (size_t)slots[b];
        if (!r.occ[s]) continue; // empty already (or named twice)
        r.tree_touch(s);
        r.occ[s] = 0;
        r.used--;
        dev.push_back(WipeRegion{r.d_pk + s * D.pk, (size_t)D.pk, 0, 1});
        dev.push_back(WipeRegion{r.d_h + s * 32, 32, 0, 1});
        dev.push_back(WipeRegion{reinterpret_cast<uint8_t *>(r.d_A) + s * a_bytes, a_bytes, 0, 1});
        dev.push_back(WipeRegion{r.d_flag + s, 1, 0, 1});
    }
    if (launch_wipe(c, dev.data(), (int)dev.size())) return -1;
    HIPCHK(stream_sync(c));
    return 0;
}

int registry_read(Ctx &c, int n, const int32_t *slots, uint8_t *state, uint8_t *pk, uint8_t *h)
{
    const KemRegistry &r = *c.registry;
    const Dims D = dims(c.P.K);
    HIPCHK(hipSetDevice(c.device));
    const hipMemcpyKind kp = pk && is_device_pointer(pk) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    const hipMemcpyKind kh = h && is_device_pointer(h) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    for (int b = 0; b < n; b++) {
        const size_t s = (size_t)slots[b];
        state[b] = r.occ[s];
        if (pk) HIPCHK(hipMemcpyAsync(pk + (size_t)b * D.pk, r.d_pk + s * D.pk, (size_t)D.pk, kp, c.stream));
        if (h) HIPCHK(hipMemcpyAsync(h + (size_t)b * 32, r.d_h + s * 32, 32, kh, c.stream));
    }
    HIPCHK(stream_sync(c));
    return 0;
}

} // namespace kosk
