// The offline bank: offline material of proofs that have no key yet, waiting in HBM.
//
// A bank ENTRY is what FRONT_OFFLINE (= FRONT_RANDOMNESS + FRONT_RANGE, mlwe_prover.cpp:4-59) leaves in one proof's row matrix: rows
// rm.f .. rm.f + 2M (f, NTT f) and rows rm.seta .. rm.seta + 2KE (the range sharings), whole rows of RS u16, packed secrets included,
// block 0 then block 1.  The bank is a ring of `capacity` such entries in one allocation.
//
//   k_bank_put  : the two row blocks of proofs 0..n-1 into n slots of the ring
//   k_bank_take : n slots into the two row blocks of proofs 0..n-1; every lane stores zeros to exactly the 16 bytes it has just loaded,
//                 behind that load, so a consumed slot is gone when the launch is: no second launch, no fill by the runtime
//
// Both kernels share one body.  An entry is cut into 16-byte units; a workgroup moves 4 x blockDim consecutive units of one proof, four
// per lane, all four loads issued before the first store, consecutive lanes on consecutive units.  The grid is (units / (4 blockDim)) x n
// with 256 lanes per workgroup where that gives 1 024 workgroups or more (1 794 for 46 Kyber-768 proofs) and one wave per workgroup
// below that (156 for one proof).  Proof b's slot is ring position (first + b) mod capacity, computed from two
// kernel arguments: the ring wraps inside a launch and no index list crosses PCIe.  Every address is a function of the unit number and the
// launch arguments alone: nothing depends on row contents, and nothing outside the addressed slots and rows is written.
#include "kosk_ctx.hpp"

#include <cstring>

namespace kosk {

#define HIPCHK(x) KOSK_HIPCHK(x)

enum { BANK_THREADS = 256, BANK_UNITS_PER_LANE = 4 }; // the most lanes of a workgroup (a launch for few proofs uses 64), units per lane

struct BankJob {
    uint8_t *P;           // row matrix of proof 0
    size_t proof_bytes;   // from one proof's row matrix to the next
    size_t off0, off1;    // where the two row blocks start in a proof's row matrix (bytes, multiples of 16)
    uint32_t units0;      // 16-byte units of block 0
    uint32_t units;       // ... of a whole entry
    uint8_t *bank;
    size_t entry_bytes;   // 16 * units
    uint32_t first, cap;  // proof b <-> slot (first + b) mod cap; first < cap, gridDim.y <= cap
};

// FULL: every unit of the workgroup lies inside the entry (block-uniform: all but the last workgroup of a proof), so the four loads go out
// back to back with nothing between them; the last workgroup guards each unit
template <bool TAKE, bool FULL>
__device__ __forceinline__ void bank_move_units(const BankJob &j, uint8_t *rows, uint8_t *ent, uint32_t u0)
{
    uint4 v[BANK_UNITS_PER_LANE];
    uint4 *in_rows[BANK_UNITS_PER_LANE], *in_bank[BANK_UNITS_PER_LANE];
#pragma unroll
    for (int i = 0; i < BANK_UNITS_PER_LANE; i++) {
        const uint32_t u = u0 + (uint32_t)i * blockDim.x;
        const uint32_t w = FULL || u < j.units ? u : 0; // (a dead lane's addresses stay inside the entry; it neither loads nor stores)
        in_rows[i] = reinterpret_cast<uint4 *>(rows + (w < j.units0 ? j.off0 + ((size_t)w << 4) : j.off1 + ((size_t)(w - j.units0) << 4)));
        in_bank[i] = reinterpret_cast<uint4 *>(ent + ((size_t)w << 4));
    }
#pragma unroll
    for (int i = 0; i < BANK_UNITS_PER_LANE; i++)
        if (FULL || u0 + (uint32_t)i * blockDim.x < j.units) v[i] = TAKE ? *in_bank[i] : *in_rows[i];
    const uint4 zero = make_uint4(0, 0, 0, 0);
#pragma unroll
    for (int i = 0; i < BANK_UNITS_PER_LANE; i++) {
        if (!FULL && u0 + (uint32_t)i * blockDim.x >= j.units) continue;
        if (TAKE) {
            *in_rows[i] = v[i];
            *in_bank[i] = zero; // the 16 bytes this lane loaded above
        } else {
            *in_bank[i] = v[i];
        }
    }
}

template <bool TAKE>
__device__ __forceinline__ void bank_move(const BankJob &j)
{
    const uint32_t b = blockIdx.y;
    uint32_t slot = j.first + b;
    if (slot >= j.cap) slot -= j.cap;
    uint8_t *rows = j.P + (size_t)b * j.proof_bytes;
    uint8_t *ent = j.bank + (size_t)slot * j.entry_bytes;
    const uint32_t per = blockDim.x * BANK_UNITS_PER_LANE;
    const uint32_t blk0 = blockIdx.x * per;
    if (blk0 + per <= j.units) bank_move_units<TAKE, true>(j, rows, ent, blk0 + threadIdx.x);
    else bank_move_units<TAKE, false>(j, rows, ent, blk0 + threadIdx.x);
}

__global__ __launch_bounds__(BANK_THREADS) void k_bank_put(BankJob j) { bank_move<false>(j); }
__global__ __launch_bounds__(BANK_THREADS) void k_bank_take(BankJob j) { bank_move<true>(j); }

// ---------------------------------------------------------------------------------------------------------------- host --

// the job for proofs 0..n-1 of the row matrix and the n ring slots from `first` on; -1 if anything would leave the rows or the ring
static int bank_job(Ctx &c, int n, int first, BankJob &j)
{
    const Params &P = c.P;
    const RowMap &rm = c.rm;
    const int r0 = 2 * P.M, r1 = 2 * P.K * P.E;
    const size_t row_bytes = (size_t)RS * sizeof(uint16_t);
    if (rm.tf != rm.f + P.M || rm.eeta != rm.seta + P.K * P.E || rm.f + r0 > rm.nrows || rm.seta + r1 > rm.nrows || row_bytes % 16 ||
        (c.proof_stride * sizeof(uint16_t)) % 16 || (reinterpret_cast<uintptr_t>(c.d_P) & 15)) {
        c.err = "internal: the offline rows are not two aligned row blocks";
        return -1;
    }
    if (!c.d_bank || n < 1 || n > c.bank_cap || n > c.call_cap || first < 0 || first >= c.bank_cap) { c.err = "internal: bank slots out of range"; return -1; }
    j.P = reinterpret_cast<uint8_t *>(c.d_P);
    j.proof_bytes = c.proof_stride * sizeof(uint16_t);
    j.off0 = (size_t)rm.f * row_bytes;
    j.off1 = (size_t)rm.seta * row_bytes;
    j.units0 = (uint32_t)((size_t)r0 * row_bytes / 16);
    j.units = (uint32_t)(bank_entry_bytes(P) / 16);
    j.bank = c.d_bank;
    j.entry_bytes = bank_entry_bytes(P);
    j.first = (uint32_t)first;
    j.cap = (uint32_t)c.bank_cap;
    return 0;
}

// Workgroups of 256 lanes where the launch has at least BANK_WIDE_MIN of them (n = 46: 1 794), else of one wave each: a launch for a
// few proofs is then four times as many workgroups (n = 1, Kyber-768: 156 instead of 39, spread over the chip's CUs by the dispatcher),
// each lane still with its four loads in flight
enum { BANK_WIDE_MIN = 1024 };
template <bool TAKE>
static int launch_bank(Ctx &c, int n, int first)
{
    BankJob j{};
    if (c.capturing) { c.err = "internal: a bank launch inside a captured segment"; return -1; }
    if (bank_job(c, n, first, j)) return -1;
    const unsigned wide = (j.units + BANK_THREADS * BANK_UNITS_PER_LANE - 1) / (BANK_THREADS * BANK_UNITS_PER_LANE);
    const unsigned threads = (unsigned long long)wide * n >= BANK_WIDE_MIN ? BANK_THREADS : 64;
    const unsigned per = threads * BANK_UNITS_PER_LANE;
    const dim3 grid((j.units + per - 1) / per, (unsigned)n);
    if (TAKE) k_bank_take<<<grid, dim3(threads), 0, c.stream>>>(j);
    else k_bank_put<<<grid, dim3(threads), 0, c.stream>>>(j);
    HIPCHK(hipGetLastError());
    c.path_n[TAKE ? PATH_BANK_TAKE : PATH_BANK_PUT]++;
    return 0;
}

// slots [first, first + n) of the ring back to zero, synchronised: what an error path owes the rule that a free slot is all zero.  Best
// effort (the stream may be the thing that failed); c.err is left as the caller set it
static void bank_zero_slots(Ctx &c, int first, int n)
{
    if (!c.d_bank || n < 1 || n > c.bank_cap) return;
    const size_t eb = bank_entry_bytes(c.P);
    const int head = n < c.bank_cap - first ? n : c.bank_cap - first;
    bool ok = hipMemsetAsync(c.d_bank + (size_t)first * eb, 0, (size_t)head * eb, c.stream) == hipSuccess;
    if (ok && n > head) ok = hipMemsetAsync(c.d_bank, 0, (size_t)(n - head) * eb, c.stream) == hipSuccess;
    if (!ok || hipStreamSynchronize(c.stream) != hipSuccess) (void)hipGetLastError();
}

void bank_release(Ctx &c)
{
    c.inv.release(Inventory::INVG_BANK);
    c.bank_cap = c.bank_ready = c.bank_head = 0;
}

void bank_note_wiped(Ctx &c)
{
    c.bank_ready = 0;
    c.bank_head = 0;
}

int bank_reserve(Ctx &c, int capacity)
{
    if (capacity < 0) { c.err = "the capacity of the bank cannot be negative"; return -1; }
    if (c.bank_ready) { c.err = "the bank is not empty: its entries are consumed or wiped before it is reserved again"; return -1; }
    HIPCHK(hipSetDevice(c.device));
    if (c.d_bank) { // nothing secret goes back to the allocator readable (free slots are zero already: this is the belt to those braces)
        if (wipe_group(c, Inventory::INVG_BANK)) return -1;
        bank_release(c);
    }
    if (!capacity) return 0;
    const size_t bytes = bank_entry_bytes(c.P) * (size_t)capacity;
    HIPCHK(c.own("d_bank", &c.d_bank, bytes, Inventory::INV_SECRET, Inventory::INVG_BANK));
    c.bank_cap = capacity;
    // a free slot is all zero, from the first one on
    if (hipMemsetAsync(c.d_bank, 0, bytes, c.stream) != hipSuccess || stream_sync(c) != hipSuccess) {
        (void)hipGetLastError();
        bank_release(c);
        c.err = "could not clear the new bank";
        return -1;
    }
    return 0;
}

int bank_fill(Ctx &c, int n, const uint8_t *tapes, size_t tape_stride, const uint8_t *seeds, size_t seed_stride, bool compact)
{
    if (n < 1 || n > c.call_cap) { c.err = "batch size out of range"; return -1; }
    if (!c.d_bank || c.bank_ready + n > c.bank_cap) { c.err = "the bank has no room for these entries (kosk_bank_reserve)"; return -1; }
    HIPCHK(hipSetDevice(c.device));
    if (stage_tape_sections(c, n, 1u << TAPE_SEC_OFFLINE, tapes, tape_stride, seeds, seed_stride, compact)) return -1;
    c.tape_segs.count = 0;
    int rc = issue_sharing_front(c, n, FRONT_OFFLINE);
    // the tape buffer holds offline sections only: whatever was staged for kosk_prove_resident before is gone
    c.tape_cur = nullptr;
    c.tape_cur_stride = 0;
    c.staged_online = false;
    if (rc) return -1;
    // behind the youngest entry; one launch also where the run of free slots passes the end of the allocation (the kernel wraps)
    const int first = (int)(((long)c.bank_head + c.bank_ready) % c.bank_cap);
    if (launch_bank<false>(c, n, first)) return -1;
    if (const hipError_t e = stream_sync(c); e != hipSuccess) { // rows may sit in slots that stay free: a free slot is all zero
        (void)hipGetLastError();
        c.err = std::string("kosk_bank_fill: ") + hipGetErrorString(e);
        bank_zero_slots(c, first, n);
        return -1;
    }
    c.bank_ready += n; // only now: a failed fill leaves the level alone
    return 0;
}

int bank_take(Ctx &c, int n)
{
    if (n < 1 || n > c.bank_ready) { c.err = c.bank_ready ? "the bank holds fewer entries than this call has proofs" : "bank is empty"; return -1; }
    const int first = c.bank_head;
    // gone from here on, whatever happens to the launch or behind it: an entry is never handed out twice
    c.bank_head = (c.bank_head + n) % c.bank_cap;
    c.bank_ready -= n;
    return launch_bank<true>(c, n, first);
}

int stage_prover_keys_banked(Ctx &c, int n, const uint8_t *sk, const uint8_t *tapes, size_t tape_stride, const uint8_t *seeds, size_t seed_stride, uint8_t *ok,
                             bool compact)
{
    if (n < 1 || n > c.call_cap) { c.err = "batch size out of range"; return -1; }
    if (!sk || !ok) { c.err = "sk records and the ok buffer are required"; return -1; }
    if (n > c.bank_ready) { c.err = c.bank_ready ? "the bank holds fewer entries than this call has proofs" : "bank is empty"; return -1; }
    HIPCHK(hipSetDevice(c.device));
    c.staged_wiped = false;
    if (stage_tape_sections(c, n, 1u << TAPE_SEC_ONLINE, tapes, tape_stride, seeds, seed_stride, compact)) return -1;
    if (witness_from_sk(c, n, sk, nullptr, ok)) return -1; // synchronised; the entries are still in the bank if this fails
    // the entry of a rejected key (ok[b] = 0) goes like any other: what is consumed does not depend on data
    if (bank_take(c, n)) return -1;
    c.staged_online = true;
    return 0;
}

// ---- diagnostic: the two kernels against the runtime's own copies and fill of the same bytes (tools/bank_rate.py) ----
int bank_timing(Ctx &c, int n, int reps, double *put_ms, double *take_ms, double *copy_ms, double *copy_fill_ms, size_t *bytes)
{
    if (n < 1 || n > c.call_cap || reps < 1) { c.err = "batch size out of range"; return -1; }
    if (c.bank_ready || n > c.bank_cap) { c.err = "the timing runs on an EMPTY bank of at least n entries"; return -1; }
    HIPCHK(hipSetDevice(c.device));
    const size_t eb = bank_entry_bytes(c.P);
    if (bytes) *bytes = eb * (size_t)n;
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct Ev { hipEvent_t *e; ~Ev() { for (int i = 0; i < 2; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } evs{ev};
    HIPCHK(hipEventCreate(&ev[0]));
    HIPCHK(hipEventCreate(&ev[1]));
    BankJob j{};
    if (bank_job(c, n, 0, j)) return -1;
    // the put leaves rows of the row matrix in slots 0..n-1 of a bank that counts them as free: they are zero again however this ends
    struct Clear { Ctx &c; int n; ~Clear() { bank_zero_slots(c, 0, n); } } clear{c, n};
    const size_t r0 = (size_t)j.units0 * 16, r1 = eb - r0;
    float ms = 0;
    auto timed = [&](double *out, const std::function<int()> &body) -> int {
        if (body()) return -1; // warm
        HIPCHK(hipEventRecord(ev[0], c.stream));
        for (int i = 0; i < reps; i++)
            if (body()) return -1;
        HIPCHK(hipEventRecord(ev[1], c.stream));
        HIPCHK(hipEventSynchronize(ev[1]));
        HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
        if (out) *out = ms / reps;
        return 0;
    };
    if (timed(put_ms, [&]() { return launch_bank<false>(c, n, 0); })) return -1;
    if (timed(take_ms, [&]() { return launch_bank<true>(c, n, 0); })) return -1;
    // the runtime's way of the same movement: two strided D2D copies (the two row blocks of every proof), and then the fill of the slots
    auto copies = [&]() -> int {
        HIPCHK(hipMemcpy2DAsync(j.P + j.off0, j.proof_bytes, c.d_bank, eb, r0, (size_t)n, hipMemcpyDeviceToDevice, c.stream));
        HIPCHK(hipMemcpy2DAsync(j.P + j.off1, j.proof_bytes, c.d_bank + r0, eb, r1, (size_t)n, hipMemcpyDeviceToDevice, c.stream));
        return 0;
    };
    if (timed(copy_ms, copies)) return -1;
    if (timed(copy_fill_ms, [&]() -> int {
            if (copies()) return -1;
            HIPCHK(hipMemsetAsync(c.d_bank, 0, eb * (size_t)n, c.stream));
            return 0;
        })) return -1;
    return 0; // (`clear` zeroes the slots and synchronises: the bank is as empty as before)
}

} // namespace kosk
