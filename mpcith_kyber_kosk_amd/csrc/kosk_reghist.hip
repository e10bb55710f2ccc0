// The registry history (kosk-reghist-v1, kosk_reghist.hpp): an append-only Merkle tree over the registry's
// mutation events, kept current in HBM by the mutating calls, with inclusion proofs for events and consistency proofs between sizes.
//   append    k_reghist_append     one block per aligned group of 1 024 inputs that the append touches: the new events' records and leaves,
//                                  then the nodes that became complete, level by level through LDS; further tiers are further launches
//   frontier  k_reghist_frontier   one wave on the wave sponge: the ragged nodes and the root of one size, a chain of popcount(n) - 1 hashes
//   proofs    k_reghist_prove      a lane pair per query: the walk of the generator, a gather of complete and ragged nodes, no hashes
// Ops, slots, fingerprints, roots and sizes are public: branches and addresses may depend on them.  A complete node is written once and
// never again: no launch communicates between its blocks, and a launch reads only what an earlier launch on the stream wrote.
#include <hip/hip_runtime.h>

#include <cstring>

#include "kosk_ctx.hpp"
#include "kosk_keccak_wave_dev.hpp"
#include "kosk_kem_dev.hpp"
#include "kosk_reghist.hpp"
#include "kosk_reghist_dev.hpp"

namespace kosk {

using namespace kem;

#define HIPCHK(x) KOSK_HIPCHK(x)

// One block, one group of a tier (reghist_group): the new events' records and leaves, the older inputs loaded, then the levels above
// (reghist_levels, kosk_reghist_dev.hpp).  All loop bounds are block-uniform.
__global__ __launch_bounds__(256) void k_reghist_append(RegHistAppendJob j)
{
    __shared__ __align__(16) uint64_t lds[(reghist::TIER_INPUTS + reghist::TIER_INPUTS / 2) * 4];
    const int tid = threadIdx.x;
    const RegHistGroup g = reghist_group(j);
    const int lo = g.lo, cnt = g.cnt;
    uint8_t *in_lvl = g.in_lvl;
    for (int i = tid; i < cnt; i += 256) {
        const int e = lo + i;
        uint64_t d[4];
        if (j.tier || e < j.s) {
            reghist_load(in_lvl + (size_t)i * 32, d);
        } else { // event e: its record, 16 bytes a store, and its leaf
            uint64_t x[4], y[4] = {0, 0, 0, 0}, st[25];
            uint32_t op, a, b = 0;
            if (j.job) {
                op = (uint32_t)j.job[2 * (e - j.s)];
                a = (uint32_t)j.job[2 * (e - j.s) + 1];
                reghist_load(j.h + (size_t)a * 32, x);
                reghist::event_state(st, j.K, x, op, a);
            } else {
                op = reghist::OP_CHECKPOINT; a = j.used; b = j.capacity;
                reghist_load(j.root_a, x);
                reghist_load(j.root_b, y);
                reghist::checkpoint_state(st, j.K, x, y, a, b);
            }
            U128 *rec = reinterpret_cast<U128 *>(j.ev + (size_t)e * reghist::EVENT_BYTES);
            rec[0] = U128{op, a, b, 0};
            rec[1] = words_u128(x[0], x[1]); rec[2] = words_u128(x[2], x[3]);
            rec[3] = words_u128(y[0], y[1]); rec[4] = words_u128(y[2], y[3]);
            perm(st);
#pragma unroll
            for (int l = 0; l < 4; l++) d[l] = st[l];
            reghist_store(in_lvl + (size_t)i * 32, d);
        }
#pragma unroll
        for (int l = 0; l < 4; l++) lds[4 * i + l] = d[l];
    }
    __syncthreads();
    reghist_levels(j, g, lds);
}

// One wave.  acc = the fold of the complete subtrees of the set bits of n from the lowest up to l: R_(l + 1), the hash of the trailing leaves
// [(n >> (l + 1)) << (l + 1), n); the root where l is the highest set bit.  Each step is one permutation that needs the one before it: the
// wave sponge at raised priority, as H(pk) in k_registry_admit.  Every branch is wave-uniform.
__global__ __launch_bounds__(64) void k_reghist_frontier(RegHistFrontierJob j)
{
    __shared__ __align__(16) uint32_t st[64];
    __shared__ __align__(16) uint64_t acc[4];
    const int lane = threadIdx.x;
    __builtin_amdgcn_s_setprio(3); // a chain is latency, not throughput
    WaveSponge sp;
    sp.setup(lane);
    bool have = false;
    if (lane < 4) {
        acc[lane] = 0;
        *reinterpret_cast<uint2 *>(j.rag + 8 * lane) = make_uint2(0, 0); // R_0: no leaf is ragged
    }
    wave_lds_handoff();
    for (int l = 0; l <= j.D; l++) {
        if ((j.n >> l) & 1) {
            const uint64_t *t = reinterpret_cast<const uint64_t *>(j.nodes + regtree::level_offset(j.D, l) + ((size_t)(j.n >> l) - 1) * 32);
            uint2 d = make_uint2(0, 0);
            if (!have) {
                if (lane < 4) d = make_uint2((uint32_t)t[lane], (uint32_t)(t[lane] >> 32));
                have = true;
            } else {
                uint32_t a = 0;
                wave_absorb_words(sp, a, [&](int w) {
                    const uint64_t v = w == 0 ? reghist::TAG0 : w == 1 ? (reghist::TAG1 | 2ULL << 56) : w < 6 ? t[w - 2] : acc[w - 6];
                    return make_uint2((uint32_t)v, (uint32_t)(v >> 32));
                }, 10, 0x06u);
                d = sp.words(a, st, 4);
            }
            wave_lds_handoff(); // acc was read above
            if (lane < 4) acc[lane] = (uint64_t)d.x | (uint64_t)d.y << 32;
            wave_lds_handoff();
        }
        if (lane < 4) {
            const uint64_t v = acc[lane];
            *reinterpret_cast<uint2 *>(j.rag + (size_t)(l + 1) * 32 + 8 * lane) = make_uint2((uint32_t)v, (uint32_t)(v >> 32));
        }
    }
}

// A lane pair per query, lane `half` copies that half of every 32-byte record.  The walk from (l, idx) at size n: level l has n >> l complete
// nodes and one ragged node iff n has a bit below l; the sibling idx ^ 1 is emitted where it is one of them.  A consistency proof starts at
// the last complete node of the old size's lowest set bit and emits that node first unless the old size is a power of two.
__global__ __launch_bounds__(256) void k_reghist_prove(RegHistProveJob j)
{
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    const long b = gid >> 1;
    const int half = (int)(gid & 1);
    if (b >= j.n) return;
    const int q = j.q[b], n = j.size, cap = (j.rec_bytes - (int)reghist::REC_NODES) / 32;
    U128 *out = reinterpret_cast<U128 *>(j.proof + (size_t)b * j.rec_bytes);
    int count = 0, l = 0, idx = q;
    bool walk = true;
    auto node_at = [&](int lv, int i) { return reinterpret_cast<const U128 *>(j.nodes + regtree::level_offset(j.D, lv) + (size_t)i * 32)[half]; };
    auto emit = [&](const U128 &v) {
        if (count < cap) out[1 + 2 * count + half] = v;
        count++;
    };
    if (j.kind == 0) {
        if (j.leaves) reinterpret_cast<U128 *>(j.leaves)[(size_t)b * 2 + half] = node_at(0, q);
    } else if (q == 0 || q == n) {
        walk = false;
    } else {
        l = __builtin_ctz((unsigned)q);
        idx = (q - 1) >> l;
        if (idx) emit(node_at(l, idx));
    }
    while (walk) {
        const int full = n >> l, rag = (n & ((1 << l) - 1)) != 0;
        if (full + rag <= 1) break;
        const int sib = idx ^ 1;
        if (sib < full) emit(node_at(l, sib));
        else if (sib == full && rag) emit(reinterpret_cast<const U128 *>(j.rag + (size_t)l * 32)[half]);
        l++;
        idx >>= 1;
    }
    if (!half) out[0] = U128{(uint32_t)count, (uint32_t)q, (uint32_t)n, 0};
    for (int c = count; c < cap; c++) out[1 + 2 * c + half] = U128{0, 0, 0, 0};
}

// ---------------------------------------------------------------------------------------------------------------- host --
// the entries whose pointers live in [lo, hi) of the registry
static void release_fields(Ctx &c, void *lo, void *hi)
{
    c.inv.release_if([lo, hi](const InvBuf &b) { return (void *)b.at >= lo && (void *)b.at < hi; });
    (void)hipGetLastError();
}

int reghist_reserve(Ctx &c, int max_events)
{
    KemRegistry &r = *c.registry;
    HIPCHK(hipSetDevice(c.device));
    if (r.hist_max) {
        HIPCHK(stream_sync(c));
        headsig_signer_release(c); // one seed serves one history: the signer goes with it
        release_fields(c, &r.d_hev, &r.d_hproof + 1);
        r.hist_max = r.hist_size = r.hstage_cap = 0;
        r.hist_frontier = -1;
    }
    if (!max_events) return 0;
    const int G = Inventory::INVG_REGISTRY; // public, all: ops, slot numbers, public fingerprints, roots and hashes of them
    if (c.own("registry.d_hev", &r.d_hev, (size_t)max_events * reghist::EVENT_BYTES, 0, G) != hipSuccess ||
        c.own("registry.d_hnode", &r.d_hnode, reghist::nodes_bytes(max_events), 0, G) != hipSuccess ||
        c.own("registry.d_hrag", &r.d_hrag, (size_t)reghist::RAGGED_SLOTS * 32, 0, G) != hipSuccess ||
        c.own("registry.d_hjob", &r.d_hjob, (size_t)KEM_CHUNK * 2 * sizeof(int32_t), 0, G) != hipSuccess) { // all or none
        release_fields(c, &r.d_hev, &r.d_hproof + 1);
        c.err = "kosk_registry_history_reserve: out of memory for the history";
        return -1;
    }
    r.hist_max = max_events;
    return 0;
}

// the tiers of one append of cnt events to a history of s; job == nullptr: the checkpoint whose operands j carries
int reghist_append_launch(Ctx &c, KemRegistry &r, RegHistAppendJob j, int s, int cnt)
{
    j.D = reghist::depth(r.hist_max); j.K = c.P.K; j.s = s; j.c = cnt; j.ev = r.d_hev; j.nodes = r.d_hnode;
    for (int t = 0; t * reghist::TIER_LEVELS <= j.D; t++) {
        const int L0 = t * reghist::TIER_LEVELS, so = s >> L0, ne = (s + cnt) >> L0;
        if (ne == so || (t && L0 >= j.D)) break; // no node of this level became complete: none above it did
        const unsigned blocks = (unsigned)(((ne - 1) >> reghist::TIER_LEVELS) - (so >> reghist::TIER_LEVELS) + 1);
        j.tier = t;
        if (j.rec && !t) {
            HIPCHK(launch_monitor_leaves(j, blocks, c.stream));
            c.path_n[PATH_MONITOR_LEAVES]++;
        } else {
            k_reghist_append<<<dim3(blocks), dim3(256), 0, c.stream>>>(j);
            HIPCHK(hipGetLastError());
            c.path_n[PATH_REGHIST_APPEND]++;
        }
        if (!t) c.path_n[PATH_REGHIST_GROUPS] += (long)blocks;
    }
    return 0;
}

int reghist_append(Ctx &c, int count, const int32_t *ops, const int32_t *slots)
{
    KemRegistry &r = *c.registry;
    if (count < 0 || count > r.hist_max - r.hist_size) { c.err = "reghist_append: the events do not fit"; return -1; }
    HIPCHK(hipSetDevice(c.device));
    std::vector<int32_t> jobs;
    for (int first = 0; first < count; first += KEM_CHUNK) {
        const int cnt = count - first < KEM_CHUNK ? count - first : (int)KEM_CHUNK;
        jobs.resize((size_t)cnt * 2);
        for (int i = 0; i < cnt; i++) { jobs[2 * (size_t)i] = ops[first + i]; jobs[2 * (size_t)i + 1] = slots[first + i]; }
        HIPCHK(hipMemcpyAsync(r.d_hjob, jobs.data(), jobs.size() * sizeof(int32_t), hipMemcpyHostToDevice, c.stream));
        RegHistAppendJob j{};
        j.job = r.d_hjob; j.h = r.d_h;
        if (reghist_append_launch(c, r, j, r.hist_size, cnt)) return -1;
        HIPCHK(stream_sync(c)); // the job list is free again, and the events are in place before the caller mutates d_h
        r.hist_size += cnt;
    }
    return 0;
}

int reghist_checkpoint(Ctx &c, int *index)
{
    KemRegistry &r = *c.registry;
    if (r.hist_size >= r.hist_max) { c.err = "kosk_registry_history_checkpoint: history is full: nothing was changed"; return -1; }
    if (registry_tree_ensure(c) || registry_sorted_ensure(c)) return -1;
    HIPCHK(hipSetDevice(c.device));
    const int D = regtree::depth(r.capacity);
    RegHistAppendJob j{};
    j.root_a = r.d_tree + regtree::level_offset(D, D); // both roots are read where they lie
    j.root_b = r.d_stree + regtree::level_offset(D, D);
    j.used = (uint32_t)r.used; j.capacity = (uint32_t)r.capacity;
    if (reghist_append_launch(c, r, j, r.hist_size, 1)) return -1;
    HIPCHK(stream_sync(c));
    if (index) *index = r.hist_size;
    r.hist_size++;
    return 0;
}

// d_hrag holds the ragged nodes and the root of `size` >= 1: queued, not synchronised; a second call at the same size launches nothing
int reghist_frontier_ensure(Ctx &c, KemRegistry &r, int size)
{
    if (r.hist_frontier == size) return 0;
    RegHistFrontierJob j{};
    j.D = reghist::depth(r.hist_max); j.n = size; j.nodes = r.d_hnode; j.rag = r.d_hrag;
    r.hist_frontier = -1;
    k_reghist_frontier<<<dim3(1), dim3(64), 0, c.stream>>>(j);
    HIPCHK(hipGetLastError());
    c.path_n[PATH_REGHIST_FRONTIER]++;
    r.hist_frontier = size;
    return 0;
}

int reghist_head(Ctx &c, KemRegistry &r, int size, uint8_t *root)
{
    HIPCHK(hipSetDevice(c.device));
    const bool dev = is_device_pointer(root);
    if (!size) {
        uint8_t o[32];
        (void)reghist::empty_root(c.P.K, o);
        if (dev) HIPCHK(hipMemcpy(root, o, 32, hipMemcpyHostToDevice));
        else memcpy(root, o, 32);
        return 0;
    }
    if (reghist_frontier_ensure(c, r, size)) return -1;
    int top = 0;
    while ((size >> top) > 1) top++;
    HIPCHK(hipMemcpyAsync(root, r.d_hrag + (size_t)(top + 1) * 32, 32, dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c.stream));
    HIPCHK(stream_sync(c));
    return 0;
}

int reghist_read(Ctx &c, int first, int n, uint8_t *events)
{
    const KemRegistry &r = *c.registry;
    HIPCHK(hipSetDevice(c.device));
    HIPCHK(hipMemcpyAsync(events, r.d_hev + (size_t)first * reghist::EVENT_BYTES, (size_t)n * reghist::EVENT_BYTES,
                          is_device_pointer(events) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c.stream));
    HIPCHK(stream_sync(c));
    return 0;
}

// the three staging buffers hold n items (rounded up to 1 024): all or none
static int staging_ensure(Ctx &c, int n)
{
    KemRegistry &r = *c.registry;
    if (n <= r.hstage_cap) return 0;
    if (r.d_hproof) HIPCHK(stream_sync(c));
    release_fields(c, &r.d_hq, &r.d_hproof + 1);
    r.hstage_cap = 0;
    const size_t N = (size_t)((n + 1023) / 1024 * 1024);
    const int G = Inventory::INVG_REGISTRY; // public: indices, sizes, copies of nodes
    if (c.own("registry.d_hq", &r.d_hq, N * sizeof(int32_t), 0, G) != hipSuccess || c.own("registry.d_hleaf", &r.d_hleaf, N * 32, 0, G) != hipSuccess ||
        c.own("registry.d_hproof", &r.d_hproof, N * reghist::consistency_bytes(r.hist_max), 0, G) != hipSuccess) {
        release_fields(c, &r.d_hq, &r.d_hproof + 1);
        c.err = "registry_history_prove: out of memory for the staging buffers";
        return -1;
    }
    r.hstage_cap = (int)N;
    return 0;
}

int reghist_prove(Ctx &c, int kind, int size, int n, const int32_t *q, uint8_t *leaves, uint8_t *records)
{
    if (n < 1 || n > KEM_CHUNK || !q || !records || !c.registry || size < 1 || size > c.registry->hist_size) { c.err = "reghist_prove: bad arguments"; return -1; }
    HIPCHK(hipSetDevice(c.device));
    if (staging_ensure(c, n)) return -1;
    const KemRegistry &r = *c.registry;
    HIPCHK(hipMemcpyAsync(r.d_hq, q, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c.stream));
    if (reghist_frontier_ensure(c, *c.registry, size)) return -1;
    RegHistProveJob j{};
    j.n = n; j.kind = kind; j.D = reghist::depth(r.hist_max); j.size = size;
    j.rec_bytes = (int)(kind ? reghist::consistency_bytes(size) : reghist::path_bytes(size));
    j.q = r.d_hq; j.nodes = r.d_hnode; j.rag = r.d_hrag; j.leaves = !kind && leaves ? r.d_hleaf : nullptr; j.proof = r.d_hproof;
    k_reghist_prove<<<dim3((unsigned)((2 * (size_t)n + 255) / 256)), dim3(256), 0, c.stream>>>(j);
    HIPCHK(hipGetLastError());
    c.path_n[PATH_REGHIST_PROVE]++;
    if (j.leaves) HIPCHK(hipMemcpyAsync(leaves, r.d_hleaf, (size_t)n * 32, is_device_pointer(leaves) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipMemcpyAsync(records, r.d_hproof, (size_t)n * j.rec_bytes, is_device_pointer(records) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c.stream));
    HIPCHK(stream_sync(c)); // the host array q is free again
    return 0;
}

} // namespace kosk
