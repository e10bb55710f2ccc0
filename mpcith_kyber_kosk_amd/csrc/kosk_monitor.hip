// The registry monitor: the third role of the transparency log.  It replays a stored event log
// (kosk-reghist-v1, kosk_reghist.hpp) onto a table of fingerprints and flags and compares, at every checkpoint, the roots, `used` and
// `capacity` that the registrar bound into the log with those of the replayed table -- in HBM, where the roots lie.
//   keys    k_monitor_keys    one lane per staged event of a segment: the record check and a 16-byte sort record (slot, position)
//   sort    regsort_network   the bitonic network of kosk_regsort.hip, unchanged: prefixes are distinct, so its tie branch is never taken
//   apply   k_monitor_apply   one lane per sorted position: the events of one slot are adjacent and in log order, so an event's state is its
//                             left neighbour's outcome or, for the first of a slot, the table's; check mode writes nothing to the table,
//                             commit mode writes every touched slot's final state
//   leaves  k_monitor_leaves  tier 0 of the history from stored records; the levels above are reghist_levels, the tiers above k_reghist_append
//   check   k_monitor_check   one wave: a checkpoint record against used, capacity and the two root nodes
// The monitor is a KemRegistry without keys (d_pk == d_A == nullptr): the slot tree, the sorted tree, the history's upper tiers and the
// frontier are the registry's own functions on it.  Everything in a log is public: branches and addresses may depend on it.
#include <hip/hip_runtime.h>

#include <cstring>

#include "kosk_ctx.hpp"
#include "kosk_kem_dev.hpp"
#include "kosk_reghist.hpp"
#include "kosk_reghist_dev.hpp"

namespace kosk {

using namespace kem;

#define HIPCHK(x) KOSK_HIPCHK(x)

enum { MON_CLASS_EVENT = 0, MON_CLASS_PAD = 1 }; // the classes of a sort record (kosk_regsort.hip): padding sorts last

__device__ __forceinline__ void monitor_report(uint32_t *word, int index, int reason) { atomicMin(word, (uint32_t)index << 8 | (uint32_t)reason); }

// Lane i < 2^lg.  A valid mutation event at position i < n: {position, slot, position, class 0}, so the 8-byte prefix is (slot << 32) |
// position and the sorted order is (slot, position).  An invalid record names no slot of the table: it is reported and becomes padding,
// {0, 0, i, class 1}, as do the positions from n on; the third word keeps padding records distinct
__global__ __launch_bounds__(256) void k_monitor_keys(MonitorJob j)
{
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >> j.lg) return;
    U128 v{0, 0, (uint32_t)i, MON_CLASS_PAD};
    if (i < j.n) {
        const U128 *ev = reinterpret_cast<const U128 *>(j.ev + (size_t)i * reghist::EVENT_BYTES);
        const U128 head = ev[0], y0 = ev[3], y1 = ev[4];
        const bool mutation = head.x == reghist::OP_ADMIT || head.x == reghist::OP_EVICT;
        if (!mutation || head.z || head.w || (y0.x | y0.y | y0.z | y0.w | y1.x | y1.y | y1.z | y1.w)) monitor_report(j.word, j.base + i, MONITOR_BAD_RECORD);
        else if (head.y >= (uint32_t)j.capacity) monitor_report(j.word, j.base + i, MONITOR_BAD_SLOT);
        else v = U128{(uint32_t)i, head.y, (uint32_t)i, MON_CLASS_EVENT};
    }
    reinterpret_cast<U128 *>(j.rec)[i] = v;
}

// Lane i < n over the sorted records.  Class-0 records come first, by (slot, position).  The state an event sees: where the record to the
// left names the same slot, that event's outcome (ADMIT: occupied with its x; EVICT: empty), whether or not it was itself valid; else the
// table's.  Check mode reports and writes nothing to the table.  Commit mode (nothing was reported): the last event of a slot's run writes
// the slot, the fingerprint as two 16-byte stores, and the block's net change of `used` goes to word[1] in one atomic
__global__ __launch_bounds__(256) void k_monitor_apply(MonitorJob j)
{
    __shared__ int delta;
    const int i = (int)(blockIdx.x * 256 + threadIdx.x);
    if (j.commit) {
        if (*j.word != MONITOR_WORD_OK) return; // block-uniform: every lane reads the same word
        if (threadIdx.x == 0) delta = 0;
        __syncthreads();
    }
    const U128 *srec = reinterpret_cast<const U128 *>(j.rec);
    U128 me{0, 0, 0, MON_CLASS_PAD};
    if (i < j.n) me = srec[i];
    if (me.w == MON_CLASS_EVENT) {
        const uint32_t slot = me.y;
        const U128 *ev = reinterpret_cast<const U128 *>(j.ev + (size_t)me.z * reghist::EVENT_BYTES);
        const uint32_t op = ev[0].x;
        const U128 x0 = ev[1], x1 = ev[2];
        if (!j.commit) {
            bool occupied;
            U128 h0, h1;
            U128 left{0, 0, 0, MON_CLASS_PAD};
            if (i > 0) left = srec[i - 1];
            if (left.w == MON_CLASS_EVENT && left.y == slot) {
                const U128 *pe = reinterpret_cast<const U128 *>(j.ev + (size_t)left.z * reghist::EVENT_BYTES);
                occupied = pe[0].x == reghist::OP_ADMIT;
                h0 = pe[1]; h1 = pe[2];
            } else {
                occupied = j.flag[slot] != 0;
                h0 = reinterpret_cast<const U128 *>(j.h + (size_t)slot * 32)[0];
                h1 = reinterpret_cast<const U128 *>(j.h + (size_t)slot * 32)[1];
            }
            const int index = j.base + (int)me.z;
            if (op == reghist::OP_ADMIT) {
                if (occupied) monitor_report(j.word, index, MONITOR_ADMIT_OCCUPIED);
            } else if (!occupied) {
                monitor_report(j.word, index, MONITOR_EVICT_EMPTY);
            } else if (((x0.x ^ h0.x) | (x0.y ^ h0.y) | (x0.z ^ h0.z) | (x0.w ^ h0.w) | (x1.x ^ h1.x) | (x1.y ^ h1.y) | (x1.z ^ h1.z) | (x1.w ^ h1.w)) != 0) {
                monitor_report(j.word, index, MONITOR_EVICT_MISMATCH);
            }
        } else {
            U128 right{0, 0, 0, MON_CLASS_PAD};
            if (i + 1 < j.n) right = srec[i + 1];
            if (!(right.w == MON_CLASS_EVENT && right.y == slot)) { // the slot's last event: no other lane touches this slot
                const int was = j.flag[slot] != 0, now = op == reghist::OP_ADMIT;
                U128 *h = reinterpret_cast<U128 *>(j.h + (size_t)slot * 32);
                h[0] = now ? x0 : U128{0, 0, 0, 0};
                h[1] = now ? x1 : U128{0, 0, 0, 0};
                j.flag[slot] = (uint8_t)now;
                if (now != was) atomicAdd(&delta, now - was);
            }
        }
    }
    if (j.commit) {
        __syncthreads();
        if (threadIdx.x == 0 && delta) atomicAdd(j.word + 1, (uint32_t)delta);
    }
}

// Tier 0 of an append whose events are stored records (j.rec, 16-byte aligned): leaf e from its record, the older inputs of the group
// loaded, then the levels above as in k_reghist_append.  No event record is kept: the monitor's history is its nodes
__global__ __launch_bounds__(256) void k_monitor_leaves(RegHistAppendJob j)
{
    __shared__ __align__(16) uint64_t lds[(reghist::TIER_INPUTS + reghist::TIER_INPUTS / 2) * 4];
    const int tid = threadIdx.x;
    const RegHistGroup g = reghist_group(j);
    for (int i = tid; i < g.cnt; i += 256) {
        const int e = g.lo + i;
        uint64_t d[4];
        if (e < j.s) {
            reghist_load(g.in_lvl + (size_t)i * 32, d);
        } else {
            const uint8_t *rec = j.rec + (size_t)(e - j.s) * reghist::EVENT_BYTES;
            const U128 head = reinterpret_cast<const U128 *>(rec)[0];
            uint64_t x[4], st[25];
            reghist_load(rec + reghist::EV_X, x);
            if (head.x == reghist::OP_CHECKPOINT) {
                uint64_t y[4];
                reghist_load(rec + reghist::EV_Y, y);
                reghist::checkpoint_state(st, j.K, x, y, head.y, head.z);
            } else {
                reghist::event_state(st, j.K, x, head.x, head.y);
            }
            perm(st);
#pragma unroll
            for (int l = 0; l < 4; l++) d[l] = st[l];
            reghist_store(g.in_lvl + (size_t)i * 32, d);
        }
#pragma unroll
        for (int l = 0; l < 4; l++) lds[4 * i + l] = d[l];
    }
    __syncthreads();
    reghist_levels(j, g, lds);
}

// One wave.  Lane l < 8 compares word l of x with the slot tree's root, lane 8 + l word l of y with the sorted tree's; the first failing
// check in the order used, capacity, slot_root, sorted_root is the reason, a non-zero reserved word comes before them all
__global__ __launch_bounds__(64) void k_monitor_check(MonitorCheckJob j)
{
    const int lane = threadIdx.x;
    const uint32_t *ev = reinterpret_cast<const uint32_t *>(j.ev);
    bool differs = false;
    if (lane < 8) differs = ev[reghist::EV_X / 4 + lane] != reinterpret_cast<const uint32_t *>(j.root_a)[lane];
    else if (lane < 16) differs = ev[reghist::EV_Y / 4 + lane - 8] != reinterpret_cast<const uint32_t *>(j.root_b)[lane - 8];
    const unsigned long long bad = __ballot(differs);
    if (lane) return;
    const int reason = ev[0] != reghist::OP_CHECKPOINT || ev[3] ? MONITOR_BAD_RECORD
                     : ev[1] != j.word[1]                      ? MONITOR_CP_USED
                     : ev[2] != (uint32_t)j.capacity           ? MONITOR_CP_CAPACITY
                     : (bad & 0xFFull)                         ? MONITOR_CP_SLOT_ROOT
                     : (bad & 0xFF00ull)                       ? MONITOR_CP_SORTED_ROOT
                                                               : MONITOR_OK;
    if (reason != MONITOR_OK) j.word[0] = (uint32_t)j.index << 8 | (uint32_t)reason;
}

hipError_t launch_monitor_keys(const MonitorJob &j, hipStream_t st)
{
    k_monitor_keys<<<dim3((unsigned)((((size_t)1 << j.lg) + 255) / 256)), dim3(256), 0, st>>>(j);
    return hipGetLastError();
}
hipError_t launch_monitor_apply(const MonitorJob &j, hipStream_t st)
{
    k_monitor_apply<<<dim3((unsigned)((j.n + 255) / 256)), dim3(256), 0, st>>>(j);
    return hipGetLastError();
}
hipError_t launch_monitor_check(const MonitorCheckJob &j, hipStream_t st)
{
    k_monitor_check<<<dim3(1), dim3(64), 0, st>>>(j);
    return hipGetLastError();
}
hipError_t launch_monitor_leaves(const RegHistAppendJob &j, unsigned blocks, hipStream_t st)
{
    k_monitor_leaves<<<dim3(blocks), dim3(256), 0, st>>>(j);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- host --
void monitor_release(Ctx &c)
{
    KemRegistry *r = c.monitor;
    if (!r) return;
    c.inv.release(Inventory::INVG_MONITOR);
    delete r;
    c.monitor = nullptr;
}

int monitor_reserve(Ctx &c, int capacity, int max_events)
{
    HIPCHK(hipSetDevice(c.device));
    if (c.monitor) {
        HIPCHK(stream_sync(c));
        monitor_release(c);
    }
    if (!capacity && !max_events) return 0;
    KemRegistry *r = new KemRegistry();
    c.monitor = r;
    r->inv_group = Inventory::INVG_MONITOR;
    const size_t N = (size_t)capacity;
    const int G = Inventory::INVG_MONITOR; // public, all: a log is public, and so is everything computed from it
    auto body = [&]() -> int {
        HIPCHK(c.own("monitor.d_h", &r->d_h, N * 32, 0, G));
        HIPCHK(c.own("monitor.d_flag", &r->d_flag, N, 0, G));
        HIPCHK(c.own("monitor.d_hnode", &r->d_hnode, reghist::nodes_bytes(max_events), 0, G));
        HIPCHK(c.own("monitor.d_hrag", &r->d_hrag, (size_t)reghist::RAGGED_SLOTS * 32, 0, G));
        HIPCHK(c.own("monitor.d_mstage", &r->d_mstage, (size_t)KEM_CHUNK * reghist::EVENT_BYTES, 0, G));
        HIPCHK(c.own("monitor.d_mrec", &r->d_mrec, (size_t)KEM_CHUNK * 16, 0, G));
        HIPCHK(c.own("monitor.d_mword", &r->d_mword, 4 * sizeof(uint32_t), 0, G));
        const uint32_t word[4] = {MONITOR_WORD_OK, 0, 0, 0};
        HIPCHK(hipMemsetAsync(r->d_h, 0, N * 32, c.stream));
        HIPCHK(hipMemsetAsync(r->d_flag, 0, N, c.stream));
        HIPCHK(hipMemcpyAsync(r->d_mword, word, sizeof(word), hipMemcpyHostToDevice, c.stream));
        HIPCHK(stream_sync(c));
        return 0;
    };
    if (body()) {
        const std::string why = c.err;
        (void)hipGetLastError();
        monitor_release(c); // nothing is left allocated
        c.err = "kosk_monitor_reserve: " + why;
        return -1;
    }
    r->capacity = capacity;
    r->hist_max = max_events;
    return 0;
}

static uint32_t le32_at(const uint8_t *p) { return reghist::le32_in(p); }

// the verdict word (and `used`) after everything queued; 1: no event was reported
static int monitor_verdict(Ctx &c, KemRegistry &r, int *bad_index, int *reason)
{
    uint32_t w[2];
    HIPCHK(hipMemcpyAsync(w, r.d_mword, sizeof(w), hipMemcpyDeviceToHost, c.stream));
    HIPCHK(stream_sync(c));
    if (w[0] == MONITOR_WORD_OK) {
        r.used = (int)w[1];
        return 1;
    }
    r.mon_failed = true;
    if (bad_index) *bad_index = (int)(w[0] >> 8);
    if (reason) *reason = (int)(w[0] & 0xFF);
    return 0;
}

// events [off, off + len) of the staged group, all of them ops other than CHECKPOINT; hv: the host's copy of the group
static int monitor_segment(Ctx &c, KemRegistry &r, const uint8_t *hv, int off, int len, int *bad_index, int *reason)
{
    int lg = 0;
    while ((1 << lg) < len) lg++;
    MonitorJob m{};
    m.n = len; m.lg = lg; m.base = r.hist_size; m.capacity = r.capacity;
    m.ev = r.d_mstage + (size_t)off * reghist::EVENT_BYTES; m.rec = r.d_mrec; m.h = r.d_h; m.flag = r.d_flag; m.word = r.d_mword;
    HIPCHK(launch_monitor_keys(m, c.stream));
    c.path_n[PATH_MONITOR_KEYS]++;
    RegSortJob s{};
    s.n = len; s.lg = lg; s.h = r.d_h; s.flag = r.d_flag; s.rec = r.d_mrec;
    if (regsort_network(c, s)) return -1;
    HIPCHK(launch_monitor_apply(m, c.stream));
    m.commit = 1;
    HIPCHK(launch_monitor_apply(m, c.stream));
    c.path_n[PATH_MONITOR_APPLY] += 2;
    const int ok = monitor_verdict(c, r, bad_index, reason);
    if (ok != 1) return ok;
    r.lookups_stale();
    for (int e = off; e < off + len; e++) r.tree_touch(le32_at(hv + (size_t)e * reghist::EVENT_BYTES + reghist::EV_A)); // accepted: every slot is one of the table's
    RegHistAppendJob a{};
    a.rec = m.ev;
    if (reghist_append_launch(c, r, a, r.hist_size, len)) return -1;
    r.hist_size += len;
    return 1;
}

// the checkpoint at position off of the staged group
static int monitor_checkpoint(Ctx &c, KemRegistry &r, int off, int *bad_index, int *reason)
{
    if (registry_tree_ensure(c, r) || registry_sorted_ensure(c, r)) return -1;
    const int D = regtree::depth(r.capacity);
    MonitorCheckJob k{};
    k.index = r.hist_size; k.capacity = r.capacity; k.ev = r.d_mstage + (size_t)off * reghist::EVENT_BYTES; k.word = r.d_mword;
    k.root_a = r.d_tree + regtree::level_offset(D, D); // both roots are read where they lie
    k.root_b = r.d_stree + regtree::level_offset(D, D);
    HIPCHK(launch_monitor_check(k, c.stream));
    c.path_n[PATH_MONITOR_CHECK]++;
    const int ok = monitor_verdict(c, r, bad_index, reason);
    if (ok != 1) return ok;
    RegHistAppendJob a{};
    a.rec = k.ev;
    if (reghist_append_launch(c, r, a, r.hist_size, 1)) return -1;
    r.hist_size++;
    return 1;
}

int monitor_feed(Ctx &c, int n, const uint8_t *events, int *bad_index, int *reason)
{
    KemRegistry &r = *c.monitor;
    HIPCHK(hipSetDevice(c.device));
    const bool dev = is_device_pointer(events);
    std::vector<uint8_t> copy;
    for (int first = 0; first < n; first += KEM_CHUNK) {
        const int cnt = n - first < KEM_CHUNK ? n - first : (int)KEM_CHUNK;
        const size_t bytes = (size_t)cnt * reghist::EVENT_BYTES;
        const uint8_t *src = events + (size_t)first * reghist::EVENT_BYTES, *hv = src;
        HIPCHK(hipMemcpyAsync(r.d_mstage, src, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c.stream));
        if (dev) { // the host cuts the group into segments and marks the touched subtrees: it reads ops and slots
            copy.resize(bytes);
            HIPCHK(hipMemcpyAsync(copy.data(), src, bytes, hipMemcpyDeviceToHost, c.stream));
            HIPCHK(stream_sync(c));
            hv = copy.data();
        }
        for (int i = 0; i < cnt;) {
            int ok;
            if (le32_at(hv + (size_t)i * reghist::EVENT_BYTES) == reghist::OP_CHECKPOINT) {
                ok = monitor_checkpoint(c, r, i, bad_index, reason);
                i++;
            } else {
                int e = i + 1;
                while (e < cnt && le32_at(hv + (size_t)e * reghist::EVENT_BYTES) != reghist::OP_CHECKPOINT) e++;
                ok = monitor_segment(c, r, hv, i, e - i, bad_index, reason);
                i = e;
            }
            if (ok != 1) {
                (void)hipStreamSynchronize(c.stream);
                return ok;
            }
        }
        HIPCHK(stream_sync(c)); // the staged group is free again, and the caller's memory is no longer read
    }
    return 1;
}

int monitor_roots(Ctx &c, uint8_t *slot_root, uint8_t *sorted_root)
{
    KemRegistry &r = *c.monitor;
    if (slot_root && registry_root(c, r, slot_root)) return -1;
    if (sorted_root && registry_sorted_root(c, r, sorted_root)) return -1;
    if (!slot_root && registry_tree_ensure(c, r)) return -1;
    if (!sorted_root && registry_sorted_ensure(c, r)) return -1;
    return 0;
}

int monitor_read(Ctx &c, int n, const int32_t *slots, uint8_t *state, uint8_t *h)
{
    const KemRegistry &r = *c.monitor;
    HIPCHK(hipSetDevice(c.device));
    const hipMemcpyKind kh = h && is_device_pointer(h) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    for (int b = 0; b < n; b++) {
        const size_t s = (size_t)slots[b];
        HIPCHK(hipMemcpyAsync(state + b, r.d_flag + s, 1, hipMemcpyDeviceToHost, c.stream));
        if (h) HIPCHK(hipMemcpyAsync(h + (size_t)b * 32, r.d_h + s * 32, 32, kh, c.stream));
    }
    HIPCHK(stream_sync(c));
    return 0;
}

} // namespace kosk
