// Erasing secrets and auditing the erasure.
//
//   k_wipe : one launch zeroes a list of regions of HBM.  A region is `count` records of `bytes` bytes, `stride` apart (one record for
//            almost every buffer; the key records keep their public head, so only the tail of each record is a region).  The regions
//            travel in the kernel arguments.  A record is cut into UNITS: unit 0 is its unaligned head and tail, stored bytewise, units
//            1.. are the 16-byte lines between them, one 16-byte store each.  Blocks are dealt over the concatenated unit count of all
//            regions, 2 048 units (32 KB) per block, consecutive lanes on consecutive lines.  Nothing outside [p, p + bytes) of a record
//            is ever addressed: every store address is derived from the record's own head / line count.
//   k_scan : counts the byte positions of a list of regions at which a needle of 16..64 bytes occurs.  One lane per position; the first
//            four bytes decide for almost every position, the rest is compared only behind them.  A block adds its count once.
//
// Both run as plain launches on the context's stream, never inside a captured segment, and their callers synchronise.
#include "kosk_ctx.hpp"

#include <cstring>

namespace kosk {

#define HIPCHK(x) KOSK_HIPCHK(x)

enum { WIPE_THREADS = 256, WIPE_UNITS_PER_LANE = 8, WIPE_UNITS_PER_BLOCK = WIPE_THREADS * WIPE_UNITS_PER_LANE };
enum { SCAN_THREADS = 256, SCAN_POS_PER_LANE = 8, SCAN_POS_PER_BLOCK = SCAN_THREADS * SCAN_POS_PER_LANE, SCAN_SLOTS = SCAN_SLOT_COUNT };

struct WipeJob {
    int n;
    uint8_t *p[WIPE_MAX_REGIONS];
    size_t stride[WIPE_MAX_REGIONS];
    uint32_t bytes_hi[WIPE_MAX_REGIONS]; // record bytes = hi << 32 | lo (kept apart: the struct stays below the kernel argument limit)
    uint32_t bytes_lo[WIPE_MAX_REGIONS];
    uint32_t count[WIPE_MAX_REGIONS];
    unsigned long long first[WIPE_MAX_REGIONS + 1]; // first unit of region r; first[n] = all units
};

struct RecShape { size_t head, lines, tail; };
__host__ __device__ static inline RecShape rec_shape(const uint8_t *p, size_t bytes)
{
    RecShape s;
    s.head = (size_t)(-(intptr_t)reinterpret_cast<uintptr_t>(p)) & 15;
    if (s.head > bytes) s.head = bytes;
    s.lines = (bytes - s.head) >> 4;
    s.tail = (bytes - s.head) & 15;
    return s;
}

__global__ __launch_bounds__(WIPE_THREADS) void k_wipe(WipeJob j)
{
    const unsigned long long u0 = (unsigned long long)blockIdx.x * WIPE_UNITS_PER_BLOCK;
    int r = 0; // the region of this block's first unit (block-uniform)
    while (r + 1 < j.n && u0 >= j.first[r + 1]) r++;
    const uint4 zero = make_uint4(0, 0, 0, 0);
    // almost every block of a large buffer lies inside the 16-byte lines of ONE single-record region (block-uniform test): eight
    // stores per lane back to back, no lookup per unit
    if (j.count[r] <= 1 && u0 > j.first[r] && u0 + WIPE_UNITS_PER_BLOCK <= j.first[r + 1]) {
        const size_t bytes = (size_t)j.bytes_hi[r] << 32 | j.bytes_lo[r];
        const RecShape s = rec_shape(j.p[r], bytes);
        uint4 *line = reinterpret_cast<uint4 *>(j.p[r] + s.head) + (size_t)(u0 - j.first[r] - 1) + threadIdx.x;
#pragma unroll
        for (int i = 0; i < WIPE_UNITS_PER_LANE; i++) line[(size_t)i * WIPE_THREADS] = zero;
        return;
    }
#pragma unroll 1
    for (int i = 0; i < WIPE_UNITS_PER_LANE; i++) {
        const unsigned long long u = u0 + (unsigned long long)i * WIPE_THREADS + threadIdx.x;
        if (u >= j.first[j.n]) return;
        while (u >= j.first[r + 1]) r++; // (empty regions have first[r] == first[r + 1] and are stepped over)
        const size_t bytes = (size_t)j.bytes_hi[r] << 32 | j.bytes_lo[r];
        unsigned long long k = u - j.first[r];
        uint8_t *rec = j.p[r];
        if (j.count[r] > 1) { // strided records: the host keeps stride a multiple of 16 and the region below 2^32 units
            const RecShape s0 = rec_shape(rec, bytes);
            const uint32_t per = (uint32_t)s0.lines + 1;
            const uint32_t b = (uint32_t)k / per;
            k = (uint32_t)k - b * per;
            rec += (size_t)b * j.stride[r];
        }
        const RecShape s = rec_shape(rec, bytes);
        if (k == 0) {
            for (size_t t = 0; t < s.head; t++) rec[t] = 0;
            uint8_t *tl = rec + s.head + (s.lines << 4);
            for (size_t t = 0; t < s.tail; t++) tl[t] = 0;
        } else {
            *reinterpret_cast<uint4 *>(rec + s.head + ((size_t)(k - 1) << 4)) = zero;
        }
    }
}

struct ScanJob {
    int n, len;
    const uint8_t *p[WIPE_MAX_REGIONS];
    unsigned long long first[WIPE_MAX_REGIONS + 1]; // first position of region r (a region of b bytes has b - len + 1 positions, or none)
    const uint8_t *needle;                          // device copy, `len` bytes
    unsigned long long *slots;                      // [SCAN_SLOTS] block counts, one add per block that found something
};

__global__ __launch_bounds__(SCAN_THREADS) void k_scan(ScanJob j)
{
    __shared__ uint8_t nd[64];
    __shared__ unsigned int found;
    if (threadIdx.x < 64) nd[threadIdx.x] = threadIdx.x < (unsigned)j.len ? j.needle[threadIdx.x] : 0;
    if (threadIdx.x == 0) found = 0;
    __syncthreads();
    const uint32_t w0 = (uint32_t)nd[0] | (uint32_t)nd[1] << 8 | (uint32_t)nd[2] << 16 | (uint32_t)nd[3] << 24;
    const unsigned long long u0 = (unsigned long long)blockIdx.x * SCAN_POS_PER_BLOCK;
    int r = 0;
    while (r + 1 < j.n && u0 >= j.first[r + 1]) r++;
    unsigned int mine = 0;
#pragma unroll 1
    for (int i = 0; i < SCAN_POS_PER_LANE; i++) {
        const unsigned long long u = u0 + (unsigned long long)i * SCAN_THREADS + threadIdx.x;
        if (u >= j.first[j.n]) break;
        while (u >= j.first[r + 1]) r++;
        const uint8_t *q = j.p[r] + (size_t)(u - j.first[r]);
        const uint32_t w = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
        if (w != w0) continue;
        int t = 4;
        while (t < j.len && q[t] == nd[t]) t++;
        mine += t == j.len;
    }
    if (mine) atomicAdd(&found, mine);
    __syncthreads();
    if (threadIdx.x == 0 && found) atomicAdd(&j.slots[blockIdx.x % SCAN_SLOTS], (unsigned long long)found);
}

// ---------------------------------------------------------------------------------------------------------------- host --

// the host's way of zeroing memory nobody reads afterwards
void host_wipe(void *p, size_t bytes)
{
    explicit_bzero(p, bytes); // glibc: a memset the compiler may not remove as a dead store
}

static void job_add(WipeJob &j, const WipeRegion &g)
{
    const int r = j.n++;
    j.p[r] = g.p;
    j.stride[r] = g.stride;
    j.bytes_hi[r] = (uint32_t)((unsigned long long)g.bytes >> 32);
    j.bytes_lo[r] = (uint32_t)g.bytes;
    j.count[r] = g.count;
    const RecShape s = rec_shape(g.p, g.bytes);
    j.first[r + 1] = j.first[r] + (g.bytes ? (unsigned long long)(s.lines + 1) * g.count : 0);
}

static int job_launch(Ctx &c, WipeJob &j)
{
    const unsigned long long units = j.first[j.n];
    if (units) {
        const unsigned long long blocks = (units + WIPE_UNITS_PER_BLOCK - 1) / WIPE_UNITS_PER_BLOCK;
        if (blocks > 0x7fffffffull) { c.err = "wipe: region list too large for one launch"; return -1; }
        k_wipe<<<dim3((unsigned)blocks), dim3(WIPE_THREADS), 0, c.stream>>>(j);
        HIPCHK(hipGetLastError());
        c.path_n[PATH_WIPE]++;
    }
    j.n = 0;
    j.first[0] = 0;
    return 0;
}

int launch_wipe(Ctx &c, const WipeRegion *regions, int n)
{
    if (c.capturing) { c.err = "internal: a wipe inside a captured segment"; return -1; }
    WipeJob j{};
    for (int i = 0; i < n; i++) {
        WipeRegion g = regions[i];
        if (!g.p || !g.bytes || !g.count) continue;
        if (g.count == 1) g.stride = 0;
        // Measured (tools/wipe_rate.py): one launch of k_wipe beats the runtime's fills of the same regions while the
        // largest of them, the row matrix, is up to about 300 MiB (0.71 of their time at max_batch 46, 0.95 at 184) and loses from
        // about 500 MiB on (1.12 at max_batch 300, 1.17 at 736): a single run of WIPE_MEMSET_BYTES or more goes to hipMemsetAsync, on
        // the same stream, everything else to k_wipe
        if (g.count == 1 && g.bytes >= (size_t)WIPE_MEMSET_BYTES) {
            HIPCHK(hipMemsetAsync(g.p, 0, g.bytes, c.stream));
            continue;
        }
        // what the kernel's strided form assumes; anything else goes record by record
        const bool strided_ok = g.count == 1 || (g.stride % 16 == 0 && g.stride >= g.bytes && (unsigned long long)(g.bytes / 16 + 2) * g.count < 0xffffffffull);
        const uint32_t pieces = strided_ok ? 1 : g.count;
        for (uint32_t k = 0; k < pieces; k++) {
            WipeRegion one = g;
            if (!strided_ok) { one.p = g.p + (size_t)k * g.stride; one.count = 1; one.stride = 0; }
            if (j.n == WIPE_MAX_REGIONS && job_launch(c, j)) return -1;
            job_add(j, one);
        }
    }
    return job_launch(c, j);
}

// ---- the inventory's two users ----

// (what a context owns of a buffer -- a view: its member's block of a per-proof buffer and its private buffers -- is the inventory's
// arithmetic: Inventory::span / secret_span / secret_regions, kosk_inventory.hpp)
int wipe_regions_list(const Ctx &c, std::vector<WipeRegion> &out, int group, unsigned skip_mask)
{
    return c.inv.secret_regions(out, group, skip_mask);
}

int wipe_group(Ctx &c, int group)
{
    std::vector<WipeRegion> dev;
    wipe_regions_list(c, dev, group);
    if (launch_wipe(c, dev.data(), (int)dev.size())) return -1;
    HIPCHK(stream_sync(c));
    return 0;
}

// A view (a cohort member) runs this on its own thread on the cohort's SHARED stream while a neighbour's run may be issuing work on it.
// That is safe because (1) views never capture graphs (ctx_make_view: use_graphs = false), so no launch of ours can land inside a
// capture, (2) the regions are the member's own block and private buffers, which no run touches while the member is not part of it
// (a member in KOSK_WIPE_CALL posts CK_ALONE; an explicit wipe must not overlap a call on the same handle), and (3) the stream
// synchronisation below merely also waits for the neighbour's work.  secret_scan() reads under the same three conditions.
int wipe_secrets(Ctx &c, bool keep_key)
{
    HIPCHK(hipSetDevice(c.device));
    std::vector<WipeRegion> dev;
    wipe_regions_list(c, dev, -1, keep_key ? 1u << Inventory::INVG_KEMKEY | 1u << Inventory::INVG_BANK | 1u << Inventory::INVG_SIGNER : 0u); // long-lived secrets stay
    // the stream may still carry this context's earlier work on these buffers: the wipe is queued behind it
    if (launch_wipe(c, dev.data(), (int)dev.size())) return -1;
    HIPCHK(stream_sync(c));
    for (const InvBuf &b : c.inv.bufs) { // page-locked staging: by the host, once nothing on the stream can write to it any more
        uint8_t *p;
        size_t rec, nrec, so, sb;
        if (!(b.flags & Inventory::INV_HOST) || !c.inv.secret_span(b, p, rec, nrec, so, sb)) continue;
        if (so == 0 && sb == rec) host_wipe(p, rec * nrec);
        else for (size_t i = 0; i < nrec; i++) host_wipe(p + i * rec + so, sb);
    }
    // what pointed at the wiped inputs: a resident proving call needs a new staging call
    if (c.tape_cur) c.staged_wiped = true;
    c.tape_cur = nullptr;
    c.tape_cur_stride = 0;
    c.tape_segs.count = 0;
    c.kg_on_host_pending = false;
    c.staged_online = false;
    if (!keep_key) bank_note_wiped(c); // every slot is zero: the bank is empty
    if (!keep_key) kem_key_note_wiped(c); // the slot's s-hat and z are zero now: it serves as a public key from here on
    if (!keep_key) headsig_note_wiped(c); // the signer's seed is zero: signing is refused until it is reserved again
    return 0;
}

static long host_count(const uint8_t *hay, size_t bytes, const uint8_t *needle, size_t len)
{
    long hits = 0;
    if (bytes < len) return 0;
    const uint8_t *p = hay, *end = hay + bytes - len + 1;
    while (p < end && (p = static_cast<const uint8_t *>(memchr(p, needle[0], (size_t)(end - p))))) {
        hits += memcmp(p, needle, len) == 0;
        p++;
    }
    return hits;
}

// d_needle: `len` bytes in HBM; h_slots / d_slots: SCAN_SLOTS counters each (page-locked host memory and HBM)
int secret_scan(Ctx &c, const uint8_t *needle, size_t len, const uint8_t *d_needle, unsigned long long *d_slots, unsigned long long *h_slots, long *hits)
{
    HIPCHK(hipSetDevice(c.device));
    HIPCHK(stream_sync(c));
    long total = 0;
    ScanJob j{};
    j.len = (int)len;
    j.needle = d_needle;
    j.slots = d_slots;
    auto flush = [&]() -> int {
        const unsigned long long pos = j.first[j.n];
        if (pos) {
            const unsigned long long blocks = (pos + SCAN_POS_PER_BLOCK - 1) / SCAN_POS_PER_BLOCK;
            if (blocks > 0x7fffffffull) { c.err = "scan: region list too large for one launch"; return -1; }
            HIPCHK(hipMemsetAsync(d_slots, 0, sizeof(unsigned long long) * SCAN_SLOTS, c.stream));
            k_scan<<<dim3((unsigned)blocks), dim3(SCAN_THREADS), 0, c.stream>>>(j);
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpyAsync(h_slots, d_slots, sizeof(unsigned long long) * SCAN_SLOTS, hipMemcpyDeviceToHost, c.stream));
            HIPCHK(stream_sync(c));
            for (int i = 0; i < SCAN_SLOTS; i++) total += (long)h_slots[i];
        }
        j.n = 0;
        j.first[0] = 0;
        return 0;
    };
    for (const InvBuf &b : c.inv.bufs) {
        uint8_t *p;
        size_t rec, nrec;
        if (!c.inv.span(b, p, rec, nrec)) continue;
        const size_t bytes = rec * nrec;
        if (b.flags & Inventory::INV_HOST) { total += host_count(p, bytes, needle, len); continue; }
        if (bytes < len) continue;
        if (j.n == WIPE_MAX_REGIONS && flush()) return -1;
        j.p[j.n] = p;
        j.first[j.n + 1] = j.first[j.n] + (bytes - len + 1);
        j.n++;
    }
    if (flush()) return -1;
    *hits = total;
    return 0;
}

} // namespace kosk
