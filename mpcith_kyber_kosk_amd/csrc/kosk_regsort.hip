// The fingerprint-sorted registry tree (kosk-regsort-v1, kosk_regsort.hpp): the occupied slots sorted by
// (fingerprint, slot), a Merkle tree over that sequence, and per query the two neighbours that straddle it -- a proof of absence -- or the
// leaf that holds it.
//   keys    k_regsort_keys    one lane per position: a 16-byte sort record (prefix of h, slot, class)
//   sort    k_regsort_tile    one block per 2 048 records: every phase of a bitonic network up to the tile, or the sub-tile steps that finish
//                             a later merge phase, in LDS
//           k_regsort_step    one or two compare-exchange steps at a distance of a tile or more, in HBM, 16-byte accesses
//   tree    k_regsort_tree    the shape of k_registry_tree (kosk_registry.hip) with this format's leaves and tag: one block per 1 024 inputs
//   proofs  k_regsort_rank    one lane per query: binary search over the records, 32-byte comparisons
//           k_regsort_prove   one lane per 16-byte piece of a proof record
// Fingerprints, flags and slot numbers are public: branches and addresses may depend on them.  An enrollee chooses its keys, so the order is
// exact for any input: where two 8-byte prefixes tie, the other 24 bytes are read from h.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "kosk_ctx.hpp"
#include "kosk_kem_dev.hpp"
#include "kosk_regsort.hpp"

namespace kosk {

using namespace kem;

#define HIPCHK(x) KOSK_HIPCHK(x)

enum { SORT_CLASS_KEY = 0, SORT_CLASS_PAD = 1 };

__device__ __forceinline__ uint64_t be64(const uint8_t *p) { return __builtin_bswap64(*reinterpret_cast<const uint64_t *>(p)); }

__global__ __launch_bounds__(256) void k_regsort_keys(RegSortJob j)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >> j.lg) return;
    U128 v{0, 0, (uint32_t)i, SORT_CLASS_PAD};
    if (i < (size_t)j.n && j.flag[i]) {
        const uint64_t p = be64(j.h + i * 32);
        v.x = (uint32_t)p; v.y = (uint32_t)(p >> 32); v.w = SORT_CLASS_KEY;
    }
    reinterpret_cast<U128 *>(j.rec)[i] = v;
}

// a sorts after b: (class, prefix, the other 24 bytes where two keys' prefixes tie, slot).  Slots are distinct, so no two records are equal
__device__ __forceinline__ bool rec_after(const U128 &a, const U128 &b, const uint8_t *h)
{
    if (a.w != b.w) return a.w > b.w;
    const uint64_t pa = (uint64_t)a.y << 32 | a.x, pb = (uint64_t)b.y << 32 | b.x;
    if (pa != pb) return pa > pb;
    if (a.w == SORT_CLASS_KEY) {
        const uint8_t *ha = h + (size_t)a.z * 32, *hb = h + (size_t)b.z * 32;
        for (int l = 8; l < 32; l += 8) {
            const uint64_t va = be64(ha + l), vb = be64(hb + l);
            if (va != vb) return va > vb;
        }
    }
    return a.z > b.z;
}

// One block, one tile of min(lg, TL) record-index bits in LDS.  phase == 0: merge phases 1 .. tile (sorted runs of a tile, their
// directions alternating); phase p above the tile: the steps at distances below a tile that finish phase p.  Record i of phase p sorts
// ascending where bit p of i is clear.  All loop bounds are block-uniform.  TL = REGSORT_TILE_LG in a block of REGSORT_TILE_THREADS; 10 and
// 12 and the smaller blocks exist for the measurement that chose them.  A pair of a step at distance 2^jj is (i, i | 2^jj):
// consecutive lanes read consecutive 16-byte records in runs of 2^jj, so a 16-lane group of a ds_read_b128 meets a bank twice at most
template <int TL> __global__ __launch_bounds__(1024) void k_regsort_tile(RegSortJob j)
{
    __shared__ __align__(16) U128 s[1 << TL];
    const int tid = threadIdx.x, nthr = blockDim.x, tl = j.lg < TL ? j.lg : TL, cnt = 1 << tl;
    const size_t base = (size_t)blockIdx.x << tl;
    U128 *g = reinterpret_cast<U128 *>(j.rec) + base;
    for (int i = tid; i < cnt; i += nthr) s[i] = g[i];
    __syncthreads();
    const int p0 = j.phase ? j.phase : 1, p1 = j.phase ? j.phase : tl;
    for (int p = p0; p <= p1; p++) {
        for (int jj = (p < tl ? p : tl) - 1; jj >= 0; jj--) {
            for (int t = tid; t < cnt / 2; t += nthr) {
                const int i = ((t >> jj) << (jj + 1)) | (t & ((1 << jj) - 1)), l = i | (1 << jj);
                const bool up = !(((base + (size_t)i) >> p) & 1);
                const U128 a = s[i], b = s[l];
                if (rec_after(a, b, j.h) == up) { s[i] = b; s[l] = a; }
            }
            __syncthreads();
        }
    }
    for (int i = tid; i < cnt; i += nthr) g[i] = s[i];
}

__device__ __forceinline__ void exchange(U128 &a, U128 &b, bool up, const uint8_t *h)
{
    if (rec_after(a, b, h) == up) { const U128 t = a; a = b; b = t; }
}

// Phase j.phase, distance 2^jg >= a tile.  TWO: also the step at 2^(jg - 1) (>= a tile as well) on the same four records in registers, so
// the records cross HBM once for two steps.  Consecutive lanes take consecutive records on every side
template <bool TWO> __global__ __launch_bounds__(256) void k_regsort_step(RegSortJob j)
{
    const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x;
    U128 *g = reinterpret_cast<U128 *>(j.rec);
    if (TWO) {
        if (t >> (j.lg - 2)) return;
        const int lo = j.jg - 1;
        const size_t d = (size_t)1 << lo, i = ((t >> lo) << (lo + 2)) | (t & (d - 1));
        const bool up = !((i >> j.phase) & 1);
        U128 a = g[i], b = g[i + d], c = g[i + 2 * d], e = g[i + 3 * d];
        exchange(a, c, up, j.h); exchange(b, e, up, j.h);
        exchange(a, b, up, j.h); exchange(c, e, up, j.h);
        g[i] = a; g[i + d] = b; g[i + 2 * d] = c; g[i + 3 * d] = e;
    } else {
        if (t >> (j.lg - 1)) return;
        const size_t d = (size_t)1 << j.jg, i = ((t >> j.jg) << (j.jg + 1)) | (t & (d - 1));
        const bool up = !((i >> j.phase) & 1);
        U128 a = g[i], b = g[i + d];
        if (rec_after(a, b, j.h) == up) { g[i] = b; g[i + d] = a; }
    }
}

// record i < n -> its slot, -1 for an empty one (kosk_regsort_order_device)
__global__ __launch_bounds__(256) void k_regsort_order(RegSortJob j)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)j.n) return;
    const U128 v = reinterpret_cast<const U128 *>(j.rec)[i];
    j.order[i] = v.w == SORT_CLASS_KEY ? (int32_t)v.z : -1;
}

// ---- the tree ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void digest_store(uint8_t *dst, const uint64_t (&d)[4])
{
    U128 *o = reinterpret_cast<U128 *>(dst);
    o[0] = U128{(uint32_t)d[0], (uint32_t)(d[0] >> 32), (uint32_t)d[1], (uint32_t)(d[1] >> 32)};
    o[1] = U128{(uint32_t)d[2], (uint32_t)(d[2] >> 32), (uint32_t)d[3], (uint32_t)(d[3] >> 32)};
}
__device__ __forceinline__ void digest_load(const uint8_t *src, uint64_t (&d)[4])
{
    const U128 a = reinterpret_cast<const U128 *>(src)[0], b = reinterpret_cast<const U128 *>(src)[1];
    d[0] = (uint64_t)a.x | (uint64_t)a.y << 32; d[1] = (uint64_t)a.z | (uint64_t)a.w << 32;
    d[2] = (uint64_t)b.x | (uint64_t)b.y << 32; d[3] = (uint64_t)b.z | (uint64_t)b.w << 32;
}

// One block, one subtree of a tier, as k_registry_tree: `cnt` <= 1 024 inputs, then `up` <= 10 levels through two LDS buffers, every node
// also to its place in the level-major tree; one sponge per lane at every level.  Block q owns inputs [1 024 q, 1 024 (q + 1)) of level
// 10 tier.  All loop bounds are block-uniform.
__global__ __launch_bounds__(256) void k_regsort_tree(RegSortTreeJob j)
{
    __shared__ __align__(16) uint64_t lds[(regtree::TIER_INPUTS + regtree::TIER_INPUTS / 2) * 4];
    const int tid = threadIdx.x, L0 = j.tier * regtree::TIER_LEVELS;
    const size_t q = blockIdx.x;
    const int cnt = j.D - L0 >= regtree::TIER_LEVELS ? (int)regtree::TIER_INPUTS : 1 << (j.D - L0);
    const int up = j.D - L0 >= regtree::TIER_LEVELS ? (int)regtree::TIER_LEVELS : j.D - L0;
    uint8_t *in_lvl = j.tree + regtree::level_offset(j.D, L0) + q * regtree::TIER_INPUTS * 32;
    for (int i = tid; i < cnt; i += 256) {
        uint64_t d[4];
        if (j.tier) {
            digest_load(in_lvl + (size_t)i * 32, d);
        } else {
            const size_t pos = q * regtree::TIER_INPUTS + (size_t)i;
            if (pos < (size_t)j.used) {
                const uint32_t slot = reinterpret_cast<const U128 *>(j.rec)[pos].z;
                uint64_t h[4], st[25];
                digest_load(j.h + (size_t)slot * 32, h);
                regsort::leaf_state(st, j.K, h, slot);
                perm(st);
#pragma unroll
                for (int l = 0; l < 4; l++) d[l] = st[l];
            } else {
#pragma unroll
                for (int l = 0; l < 4; l++) d[l] = j.pad[l];
            }
            digest_store(in_lvl + (size_t)i * 32, d);
        }
#pragma unroll
        for (int l = 0; l < 4; l++) lds[4 * i + l] = d[l];
    }
    __syncthreads();
    int in = 0, out = regtree::TIER_INPUTS * 4; // word offsets of the two buffers
    for (int lv = 1; lv <= up; lv++) {
        const int m = cnt >> lv;
        uint8_t *dst = j.tree + regtree::level_offset(j.D, L0 + lv) + q * (size_t)(regtree::TIER_INPUTS >> lv) * 32;
        for (int i = tid; i < m; i += 256) {
            uint64_t l[4], r[4], st[25];
#pragma unroll
            for (int w = 0; w < 4; w++) { l[w] = lds[in + 8 * i + w]; r[w] = lds[in + 8 * i + 4 + w]; }
            regsort::node_state(st, l, r);
            perm(st);
#pragma unroll
            for (int w = 0; w < 4; w++) { l[w] = st[w]; lds[out + 4 * i + w] = st[w]; }
            digest_store(dst + (size_t)i * 32, l);
        }
        __syncthreads();
        const int t = in; in = out; out = t;
    }
}

// ---- proofs ------------------------------------------------------------------------------------------------------------
// h[slot] against x as 32 bytes in memcmp order: < 0, 0, > 0
__device__ __forceinline__ int fingerprint_cmp(const uint8_t *h, const uint8_t *x)
{
    for (int l = 0; l < 32; l += 8) {
        const uint64_t a = be64(h + l), b = be64(x + l);
        if (a != b) return a < b ? -1 : 1;
    }
    return 0;
}

// One lane per query: lb = the number of entries below x, over the first `used` records; present = entry lb holds x (the lowest such slot:
// equal fingerprints lie in slot order)
__global__ __launch_bounds__(64) void k_regsort_rank(RegSortProveJob j)
{
    const long b = (long)blockIdx.x * 64 + threadIdx.x;
    if (b >= j.n) return;
    const uint8_t *x = j.q + (size_t)b * 32;
    const U128 *rec = reinterpret_cast<const U128 *>(j.rec);
    int lo = 0, hi = j.used;
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (fingerprint_cmp(j.h + (size_t)rec[mid].z * 32, x) < 0) lo = mid + 1;
        else hi = mid;
    }
    const bool present = lo < j.used && fingerprint_cmp(j.h + (size_t)rec[lo].z * 32, x) == 0;
    j.rank[2 * b] = lo;
    j.rank[2 * b + 1] = present;
    j.kind[b] = present ? regsort::KIND_PRESENT : regsort::KIND_ABSENT;
}

// One lane per 16-byte piece of a proof record (kosk_regsort.hpp): piece 0 the header, 1..2 h_l, 3..4 h_r, then path_l and path_r, two
// pieces a level.  Parts the record does not use are zero
__global__ __launch_bounds__(256) void k_regsort_prove(RegSortProveJob j)
{
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const int per = 5 + 4 * j.D;
    if (gid >= (long)per * j.n) return;
    const long b = gid / per;
    const int piece = (int)(gid - b * per);
    const int lb = j.rank[2 * b];
    const bool present = j.rank[2 * b + 1] != 0;
    const long P = 1L << j.D;
    const U128 *rec = reinterpret_cast<const U128 *>(j.rec);
    const bool left = present || lb >= 1, right = !present && lb < P, key = right && lb < j.used;
    const long pos_l = present ? lb : lb - 1L, pos_r = lb;
    U128 v{0, 0, 0, 0};
    if (piece == 0) {
        v.x = (uint32_t)(int32_t)(left ? pos_l : -1);
        v.y = left ? rec[pos_l].z : 0;
        v.z = key ? rec[pos_r].z : 0;
        v.w = (left ? regsort::FLAG_LEFT : 0) | (right ? regsort::FLAG_RIGHT : 0) | (key ? regsort::FLAG_RIGHT_KEY : 0) | (present ? regsort::FLAG_PRESENT : 0);
    } else if (piece < 5) {
        const int side = (piece - 1) >> 1, half = (piece - 1) & 1;
        if (side == 0 ? left : key) v = reinterpret_cast<const U128 *>(j.h + (size_t)rec[side == 0 ? pos_l : pos_r].z * 32)[half];
    } else {
        const int r = piece - 5, side = r >= 2 * j.D, l = (r - (side ? 2 * j.D : 0)) >> 1, half = r & 1;
        if (side == 0 ? left : right) {
            const size_t pos = (size_t)(side == 0 ? pos_l : pos_r);
            v = reinterpret_cast<const U128 *>(j.tree + regtree::level_offset(j.D, l) + ((pos >> l) ^ 1) * 32)[half];
        }
    }
    reinterpret_cast<U128 *>(j.proof)[(size_t)b * per + piece] = v;
}

// ---------------------------------------------------------------------------------------------------------------- host --
// KOSK_DEBUG_REGSORT_STEP2=0 runs every step above the tile in a launch of its own (1, the default: two steps a launch where two are left);
// read at every sort, so a measurement can alternate the settings in one process
static bool regsort_step2()
{
    const char *e = getenv("KOSK_DEBUG_REGSORT_STEP2");
    return e ? atoi(e) != 0 : true;
}

// KOSK_DEBUG_REGSORT_TILE_LG=10 / 12 sorts with tiles of 1 024 / 4 096 records (16 / 64 KB of LDS); read at every sort
static int regsort_tile_lg()
{
    const char *e = getenv("KOSK_DEBUG_REGSORT_TILE_LG");
    const int v = e ? atoi(e) : (int)REGSORT_TILE_LG;
    return v == 10 || v == 12 ? v : (int)REGSORT_TILE_LG;
}

static unsigned blocks_of(size_t lanes, unsigned per) { return (unsigned)((lanes + per - 1) / per); }

// KOSK_DEBUG_REGSORT_TILE_THREADS=256 / 512 / 1024: the block size of k_regsort_tile (a lane takes 2^(tile - 1) / threads pairs a step)
static unsigned regsort_tile_threads()
{
    const char *e = getenv("KOSK_DEBUG_REGSORT_TILE_THREADS");
    const int v = e ? atoi(e) : (int)REGSORT_TILE_THREADS;
    return v == 256 || v == 512 || v == 1024 ? (unsigned)v : (unsigned)REGSORT_TILE_THREADS;
}

static hipError_t launch_tile(const RegSortJob &j, int T, unsigned tiles, hipStream_t st)
{
    const dim3 block(regsort_tile_threads());
    if (T == 10) k_regsort_tile<10><<<dim3(tiles), block, 0, st>>>(j);
    else if (T == 12) k_regsort_tile<12><<<dim3(tiles), block, 0, st>>>(j);
    else k_regsort_tile<REGSORT_TILE_LG><<<dim3(tiles), block, 0, st>>>(j);
    return hipGetLastError();
}

int regsort_sort(Ctx &c, const RegSortJob &j)
{
    k_regsort_keys<<<dim3(blocks_of((size_t)1 << j.lg, 256)), dim3(256), 0, c.stream>>>(j);
    HIPCHK(hipGetLastError());
    c.path_n[PATH_REGSORT_SORT]++;
    return regsort_network(c, j);
}

int regsort_network(Ctx &c, const RegSortJob &job)
{
    RegSortJob j = job;
    const int T = regsort_tile_lg();
    const size_t N = (size_t)1 << j.lg;
    const unsigned tiles = j.lg > T ? 1u << (j.lg - T) : 1u;
    const bool two = regsort_step2();
    j.phase = 0;
    HIPCHK(launch_tile(j, T, tiles, c.stream));
    c.path_n[PATH_REGSORT_SORT]++;
    for (int p = T + 1; p <= j.lg; p++) {
        j.phase = p;
        for (int jg = p - 1; jg >= T;) {
            j.jg = jg;
            if (two && jg - 1 >= T) {
                k_regsort_step<true><<<dim3(blocks_of(N / 4, 256)), dim3(256), 0, c.stream>>>(j);
                jg -= 2;
            } else {
                k_regsort_step<false><<<dim3(blocks_of(N / 2, 256)), dim3(256), 0, c.stream>>>(j);
                jg -= 1;
            }
            HIPCHK(hipGetLastError());
            c.path_n[PATH_REGSORT_SORT]++;
        }
        HIPCHK(launch_tile(j, T, tiles, c.stream));
        c.path_n[PATH_REGSORT_SORT]++;
    }
    return 0;
}

// the entries whose pointers live in [lo, hi) of the registry
static void release_fields(Ctx &c, void *lo, void *hi)
{
    c.inv.release_if([lo, hi](const InvBuf &b) { return (void *)b.at >= lo && (void *)b.at < hi; });
    (void)hipGetLastError();
}

int registry_sorted_ensure(Ctx &c, KemRegistry &r)
{
    if (r.sorted_valid) return 0;
    HIPCHK(hipSetDevice(c.device));
    const int D = regtree::depth(r.capacity), T = regtree::tiers(D);
    if (!r.d_stree) { // public, both: slot numbers, prefixes and hashes of public fingerprints
        const int G = r.inv_group;
        if (c.own(r.buf_name("registry.d_srec", "monitor.d_srec"), &r.d_srec, (size_t)16 << D, 0, G) != hipSuccess ||
            c.own(r.buf_name("registry.d_stree", "monitor.d_stree"), &r.d_stree, regtree::tree_bytes(r.capacity), 0, G) != hipSuccess) { // both or neither
            release_fields(c, &r.d_srec, &r.d_stree + 1);
            c.err = "registry_sorted_ensure: out of memory for the sorted tree";
            return -1;
        }
    }
    RegSortJob s{};
    s.n = r.capacity; s.lg = D; s.h = r.d_h; s.flag = r.d_flag; s.rec = r.d_srec;
    if (regsort_sort(c, s)) return -1;
    RegSortTreeJob j{};
    j.D = D; j.K = c.P.K; j.used = r.used; j.h = r.d_h; j.rec = r.d_srec; j.tree = r.d_stree;
    uint8_t z[32];
    (void)regsort::leaf(c.P.K, nullptr, 0, z);
    memcpy(j.pad, z, 32);
    for (int t = 0; t < T; t++) {
        j.tier = t;
        const int above = D - t * regtree::TIER_LEVELS;
        k_regsort_tree<<<dim3(above > regtree::TIER_LEVELS ? 1u << (above - regtree::TIER_LEVELS) : 1u), dim3(256), 0, c.stream>>>(j);
        HIPCHK(hipGetLastError());
        c.path_n[PATH_REGSORT_TREE]++;
    }
    // records staged from the earlier state go with it: after an eviction and this rebuild no copy of the evicted fingerprint is left
    if (r.d_sproof) HIPCHK(hipMemsetAsync(r.d_sproof, 0, (size_t)r.sproof_cap * regsort::proof_bytes(D), c.stream));
    HIPCHK(stream_sync(c));
    r.sorted_valid = true;
    return 0;
}

int registry_sorted_root(Ctx &c, KemRegistry &r, uint8_t *root)
{
    if (registry_sorted_ensure(c, r)) return -1;
    const int D = regtree::depth(r.capacity);
    HIPCHK(hipMemcpyAsync(root, r.d_stree + regtree::level_offset(D, D), 32, is_device_pointer(root) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c.stream));
    HIPCHK(stream_sync(c));
    return 0;
}

// the four staging buffers hold n items (rounded up to 1 024): all or none
static int regsort_staging_ensure(Ctx &c, int n)
{
    KemRegistry &r = *c.registry;
    if (n <= r.sproof_cap) return 0;
    HIPCHK(hipSetDevice(c.device));
    if (r.d_sproof) HIPCHK(stream_sync(c));
    release_fields(c, &r.d_sq, &r.d_sproof + 1);
    r.sproof_cap = 0;
    const size_t N = (size_t)((n + 1023) / 1024 * 1024), rec = regsort::proof_bytes(regtree::depth(r.capacity));
    const int G = Inventory::INVG_REGISTRY; // public: query fingerprints (zeroed after each call), ranks, kinds, copies of fingerprints and nodes
    if (c.own("registry.d_sq", &r.d_sq, N * 32, 0, G) != hipSuccess || c.own("registry.d_srank", &r.d_srank, N * 2 * sizeof(int32_t), 0, G) != hipSuccess ||
        c.own("registry.d_skind", &r.d_skind, N, 0, G) != hipSuccess || c.own("registry.d_sproof", &r.d_sproof, N * rec, 0, G) != hipSuccess) {
        release_fields(c, &r.d_sq, &r.d_sproof + 1);
        c.err = "registry_prove_absent: out of memory for the staging buffers";
        return -1;
    }
    r.sproof_cap = (int)N;
    return 0;
}

int registry_prove_absent(Ctx &c, int n, const uint8_t *h, uint8_t *kind, uint8_t *records)
{
    if (n < 1 || n > KEM_CHUNK || !h || !kind || !records || !c.registry) { c.err = "registry_prove_absent: bad arguments"; return -1; }
    if (registry_sorted_ensure(c)) return -1;
    if (regsort_staging_ensure(c, n)) return -1;
    const KemRegistry &r = *c.registry;
    const int D = regtree::depth(r.capacity);
    const size_t rec = regsort::proof_bytes(D);
    HIPCHK(hipSetDevice(c.device));
    HIPCHK(hipMemcpyAsync(r.d_sq, h, (size_t)n * 32, is_device_pointer(h) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c.stream));
    RegSortProveJob j{};
    j.n = n; j.D = D; j.used = r.used; j.q = r.d_sq; j.h = r.d_h; j.rec = r.d_srec; j.tree = r.d_stree;
    j.rank = r.d_srank; j.kind = r.d_skind; j.proof = r.d_sproof;
    k_regsort_rank<<<dim3(blocks_of((size_t)n, 64)), dim3(64), 0, c.stream>>>(j);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemsetAsync(r.d_sq, 0, (size_t)n * 32, c.stream)); // the staged queries go, as in kem_registry_find
    k_regsort_prove<<<dim3(blocks_of((size_t)n * (5 + 4 * D), 256)), dim3(256), 0, c.stream>>>(j);
    HIPCHK(hipGetLastError());
    c.path_n[PATH_REGSORT_PROVE]++;
    HIPCHK(hipMemcpyAsync(kind, r.d_skind, (size_t)n, is_device_pointer(kind) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipMemcpyAsync(records, r.d_sproof, (size_t)n * rec, is_device_pointer(records) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c.stream));
    HIPCHK(stream_sync(c));
    return 0;
}

int regsort_order_device(Ctx &c, int n, const uint8_t *d_h, const uint8_t *d_flag, int32_t *d_order)
{
    HIPCHK(hipSetDevice(c.device));
    int lg = 0;
    while (((size_t)1 << lg) < (size_t)n) lg++;
    uint8_t *rec = nullptr; // comes and goes with the call
    if (c.own("regsort.order_rec", &rec, (size_t)16 << lg, 0, Inventory::INVG_REGISTRY) != hipSuccess) {
        (void)hipGetLastError();
        c.err = "kosk_regsort_order_device: out of memory for the records";
        return -1;
    }
    auto body = [&]() -> int {
        RegSortJob s{};
        s.n = n; s.lg = lg; s.h = d_h; s.flag = d_flag; s.rec = rec; s.order = d_order;
        if (regsort_sort(c, s)) return -1;
        k_regsort_order<<<dim3(blocks_of((size_t)n, 256)), dim3(256), 0, c.stream>>>(s);
        HIPCHK(hipGetLastError());
        HIPCHK(stream_sync(c));
        return 0;
    };
    const int rc = body();
    if (rc) (void)hipStreamSynchronize(c.stream);
    release_fields(c, &rec, &rec + 1);
    return rc;
}

} // namespace kosk
