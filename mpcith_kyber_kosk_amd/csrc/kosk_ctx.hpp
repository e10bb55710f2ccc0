// Library context: constant tables + HBM workspace for up to max_batch proofs
// in flight, and the batched prove / verify pipelines built on kosk_kernels.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <functional>
#include <vector>

#include "kosk_device.hpp"
#include "kosk_host.hpp"
#include "kosk_inventory.hpp"
#include "kosk_params.hpp"

// Every HIP call of the host code goes through this (needs a `Ctx &c` in scope, returns -1 from the enclosing function).
// HIP keeps the last error per host thread until somebody reads it, and every kernel launcher reports hipGetLastError():
// a failure reported here is consumed here, so that it cannot come back as the "result" of the next, healthy launch on this
// thread (r3: a failed kosk_create on a bad device ordinal made the next handle's first launch fail).
#define KOSK_HIPCHK(x)                                                      \
    do {                                                                    \
        hipError_t e_ = (x);                                                \
        if (e_ != hipSuccess) {                                             \
            (void)hipGetLastError();                                        \
            c.err = std::string(#x) + ": " + hipGetErrorString(e_);         \
            return -1;                                                      \
        }                                                                   \
    } while (0)

namespace kosk {

typedef void (*randombytes_fn)(void *user, uint8_t *out, size_t len);
// called on the calling thread when a commitment round's digest table [n][1454][32] is complete in HBM (the stream may already run
// the next segment, which never writes the tables):
// role 0 prover / 1 verifier, round 0 Tcomm / 1 view commitments
typedef void (*round_fn)(void *user, int role, int round, const void *d_digests, size_t bytes);

// key generation folded into the prover's first segment (kyber_verifiable_keygen as ONE resident call)
struct KeygenIn {
    const uint8_t *tapes; // host or device memory; nullptr: the randombytes callback
    size_t tape_stride;
    uint8_t *pk, *sk;     // host, n records each
    // a merged call (kosk_combine.hpp): several callers' batches back to back in one pipeline run.  This segment covers the
    // next `count` proofs (0: all the remaining ones), `next` the ones behind it
    int count = 0;
    const KeygenIn *next = nullptr;
    // this caller's own round hook (a merged run fires every member's hook with that member's block of the digest table; an
    // unmerged call leaves these null and the context's round_hook fires for the whole batch)
    round_fn hook = nullptr;
    void *hook_user = nullptr;
    // seeded proving: `seeds` != nullptr (host or device memory, seed_stride >= 32 apart) replaces `tapes` -- this caller's tapes are
    // expanded from its 32-byte seeds into the context's own tape buffer (kosk-seedtape-v1, k_tape_expand)
    const uint8_t *seeds = nullptr;
    size_t seed_stride = 0;
    // a banked key generation (unmerged only): bit s set = section s of the tapes is made resident and nothing else of them is read
    // (stage_tape_sections); 0: whole tapes
    unsigned sections = 0;
    bool sections_compact = false; // the records hold exactly those sections back to back (drawn randomness), not whole tapes
};
// the verifier's per-caller parts of a merged call: `count` proofs each, own key source and own result bytes
struct VerifySeg {
    int count;
    const uint8_t *pk; // pk_mode 1: this caller's public keys (host or device memory)
    uint8_t *ok;
    const VerifySeg *next = nullptr;
    round_fn hook = nullptr; // as KeygenIn::hook
    void *hook_user = nullptr;
};

enum Phase { PH_HOST_PRE = 0, PH_GPU_COMMIT, PH_FS_ALPHA, PH_GPU_RELATION, PH_FS_OPEN, PH_GPU_ASSEMBLE, PH_D2H,
             // host time spent issuing each segment (part of the GPU phases above) and the verifier's phases
             PH_P1_ISSUE, PH_P2_ISSUE, PH_P3_ISSUE, PH_V1_ISSUE, PH_V1_WAIT, PH_V_FS_ALPHA, PH_V2_ISSUE, PH_V2_WAIT, PH_V_FS_OPEN,
             PH_COUNT };

// HIP-event timing of individual launches on the ctx stream (bench.py roofline leg)
enum ProfId { PR_HASH_TCOMM = 0, PR_HASH_VIEW, PR_GEMM_EXPAND1, PR_GEMM_EXPAND2, PR_LINCOMB, PR_NTT_F, PR_ASSEMBLE,
              PR_V_HASH_TCOMM, PR_V_HASH_VIEW, PR_V_INTERP_BUILD, PR_V_GEMM_INTERP, PR_V_GEMM_EXPAND, PR_V_GEMM_RECON,
              PR_V_LINCOMB, PR_FS_ALPHA, PR_FS_OPENED, PR_V_FS_ALPHA, PR_V_FS_OPENED, PR_COUNT };

enum PathId { PATH_HASH_DMA = 0, PATH_HASH_PLAIN, PATH_TABLE_GEMM, PATH_LIMB_GEMM, PATH_COPY_DIRECT, PATH_COPY_STAGED,
              PATH_GRAPH_REPLAY, PATH_DIGEST_COPY, PATH_SMALL_COPY_KERNEL, PATH_FS_DEVICE, PATH_FS_HOST, PATH_TAPE_EXPAND, PATH_KEM_ENC, PATH_KEM_DEC, PATH_DENSE_FILL, PATH_KEM_KEYPAIR, PATH_KEM_CHECK, PATH_KEYSEED, PATH_WIPE,
              PATH_KEM_KEY_SETUP, PATH_KEM_ENC_KEY, PATH_KEM_DEC_KEY, PATH_DENSE_CHECK, PATH_DENSE2_FILL, PATH_DENSE2_CHECK, PATH_BANK_PUT, PATH_BANK_TAKE, PATH_REGISTRY_ADMIT, PATH_KEM_ENC_SLOTS,
              PATH_REGISTRY_INDEX, PATH_REGISTRY_FIND, PATH_KEM_ENC_PEERS, PATH_REGISTRY_TREE, PATH_REGISTRY_SUBTREES, PATH_REGISTRY_PATH,
              PATH_REGSORT_SORT, PATH_REGSORT_TREE, PATH_REGSORT_PROVE, PATH_REGHIST_APPEND, PATH_REGHIST_GROUPS, PATH_REGHIST_FRONTIER, PATH_REGHIST_PROVE,
              PATH_MONITOR_KEYS, PATH_MONITOR_APPLY, PATH_MONITOR_LEAVES, PATH_MONITOR_CHECK,
              PATH_REGTREE_CHECK, PATH_REGSORT_CHECK, PATH_KEM_ENC_PROVEN,
              PATH_HEADSIG_LEAVES, PATH_HEADSIG_TREE, PATH_HEADSIG_SIGN, PATH_HEADSIG_VERIFY,
              PATH_COUNT };

struct GemmTable {
    uint8_t *dfrag = nullptr; // limb matrix (kosk_device.hpp) in fragment-linear tile order (pack_frag_table)
    int M = 0, Mpad = 0, KS = 0; // KS = k-steps of 64: 7 (407-wide) or 13 (813-wide)
};

// source rows / destination rows of one mod-q GEMM
struct GemmSrc {
    const uint16_t *src;
    size_t gstride;
    const int16_t *rows;
    int rstride, koff;
    // every u16 of the rows is a canonical field element (< q): true for everything the pipelines produce (the verifier folds what it
    // takes from a proof image before it reaches the row matrix); 0 for caller data of the kernel-level entry points, which is
    // folded while it is converted (the slower conversion)
    int canonical = 1;
};
struct GemmDst {
    uint16_t *C;
    size_t gstride;
    const int16_t *rows;
    int rstride, off;
};

// compact wire format (kosk_compact.hip)
struct CompactField {
    uint32_t src_off, dst_off, n; // image offset, compact offset, u16 values (or bytes when raw)
    int raw;
};
struct CompactPlan {
    CompactField f[NFIELDS];
    size_t bytes;
};
CompactPlan make_compact_plan(const Params &P);
int compact_encode(const Params &P, const uint8_t *img, uint8_t *out); // -1: a value >= 4096
void compact_decode(const Params &P, const uint8_t *in, uint8_t *img);
// dense wire format kosk-dense-v1 (kosk_dense.hip): the compact layout with rows 0..406 only of the seven low-degree fields
// kosk-dense-v2 (fmt = 4, FMT_DENSE2 below): the eta-gate fields keep rows 0..150 and the two u fields rows 0..556
CompactPlan make_dense_plan(const Params &P, int fmt = 2);
int dense_encode(const Params &P, const uint8_t *img, uint8_t *out, int fmt = 2); // -1: a stored value >= 4096; -2: malformed I, or a dropped row that is not the refill
int dense_decode(const Params &P, const uint8_t *in, uint8_t *img, int fmt = 2);  // 0, or 1: malformed I (the dropped rows of the format's fields left zero)

struct TcWs;  // HBM workspace of kosk_transcode_batch (kosk_compact.hip)
struct KemWs; // HBM workspace of the KEM calls (kosk_kem_kernels.hip)
struct KemKey; // the resident key of the one-key KEM calls (kosk_kem_kernels.hip)
struct KemRegistry; // the table of admitted keys (kosk_registry.hip)
enum { KEM_CHUNK = 16384,    // items per launch group of the KEM calls; larger calls are chunked
       KEM_WAVE_MAX = 1024 }; // launch groups of up to this many items (one wave per SIMD) run their long one-lane-per-item chains on a wave sponge, one wave per item

// ---- the context, in three parts by what a VIEW does with a field ----
// A view of a context (kosk_combine.hpp) runs the pipeline on proofs [view_first, view_first + max_batch) of the context it was made from
// (the arena) while other views work on other proofs of it.  ctx_make_view builds one by rule, part by part:
//   CtxShared  : taken from the arena as it is -- what depends only on (device, kyber_k, options): constants, strides, the constant tables
//                and the verifier's, the knobs, the stream.  The arena owns the tables; a view only points at them.
//   CtxBlock   : the per-proof buffers' pointers and nothing else.  A view gets each one `view_first` records further
//                (Inventory::view_of), as windows it does not own.
//   CtxPrivate : every context, owner or view, starts these from their defaults: errors, events, workers, counters, the state of the
//                calls in flight, and every buffer a context allocates for itself on first use (through its own inventory).
// A NEW FIELD goes where its answer to "what must a cohort member see?" puts it: the arena's value (Shared), its own block of the arena's
// buffer (Block; allocate it with INV_PER_PROOF), or a fresh one of its own (Private).  If in doubt, Private: a member that lacks something
// fails loudly, a member that shares something by accident frees it twice or shows its secrets to a neighbour.
struct CtxShared {
    int device = 0;
    Params P{};
    RowMap rm{};
    // one HIP stream per cohort, shared on purpose.  In steady state a cohort has one merged run in flight, so nothing is lost -- and the
    // number of streams that carry work stays at the number of cohorts: ROCm deals streams to its (four) hardware queues in creation
    // order, and with a stream per member the streams of the run leaders of three cohorts of three all landed on the SAME hardware queue
    // (measured: 138-proof runs took 2.8 ms instead of 1.6).  Calls end with a stream synchronisation, so members never leave work behind
    // for each other.  Destroyed by the context that created it
    hipStream_t stream = nullptr;
    int base_threads = 1; // host threads of a call of own_batch proofs (a merged run uses base_threads x members)
    int n_simd = 1024;    // SIMDs of the device (4 per CU)

    // constant tables (HBM, L2-resident while in use)
    GemmTable t_expand, t_recon_d, t_recon_2d;
    int16_t *d_fresh_rows = nullptr, *d_gemm1_rows = nullptr, *d_gemm2_rows = nullptr;
    int n_gemm1 = 0, n_gemm2 = 0;
    int32_t *d_off = nullptr; // NTT offset tables, see build_tables()
    int off_ntt1_src = 0, off_ntt1_dst = 0, n_ntt1 = 0; // NTT(f_i) -> Tf_i and NTT(s_i) -> shat_i in one launch
    int off_sr_er = 0, off_nttsr_er = 0;
    FieldDesc *d_fields = nullptr;
    int16_t *d_rowtab = nullptr;
    AsmGroup *d_asm_groups = nullptr; // the grouped image kernel's tables (build_tables)
    AsmElem *d_asm_elems = nullptr;
    int n_asm_groups = 0;
    int nfields = 0;
    std::vector<FieldDesc> h_fields;
    std::vector<int16_t> h_rowtab;
    int16_t *d_lin_rows = nullptr; // [2][128] output rows of the lincomb GEMM (beta/r, gamma/NTT_r)

    // strides of the per-batch workspace
    size_t proof_stride = 0; // u16 per proof in the row matrix
    size_t tape_stride = 0, image_stride = 0, key_stride = 0, se_stride = 0;
    int sel_stride = 0;
    size_t kg_rec = 0, sb_bytes = 0; // the key record (CtxBlock::d_kg)
    size_t pk_stride = 0, sb_stride = 0;

    // the verifier's tables and plans (allocated with the workspace on first use, kosk_verify.cpp; verify_ready is set last)
    bool verify_ready = false;
    size_t o_stride = 0;
    uint16_t *d_inv = nullptr;       // [Q] field inverses
    FieldDesc *d_vfields = nullptr;  // proof image -> rows (verifier row assignment)
    int16_t *d_vrowtab = nullptr;
    int n_vfields = 0;
    FieldPlan vplan{}, pplan{}; // block -> (field, chunk) maps of the disassemble / assemble kernels
    int16_t *d_rows_bg = nullptr;    // beta_0..69, gamma_0..69
    int16_t *d_rows_isrc = nullptr, *d_rows_idst = nullptr; // degree-d interpolations: given rows -> recomputed rows
    int16_t *d_rows_u = nullptr;     // us / ue rows (degree 2d)
    int n_interp_d = 0, n_interp_2d = 0;
    uint16_t *d_fact = nullptr, *d_invfact = nullptr;
    uint16_t *d_invlimb = nullptr;

    // ---- knobs ----
    // KOSK_WAIT_NAP (default 1 since round 5; 0: spin throughout): the long host waits of the resident calls (six per step: the GPU
    // phases between the host's rounds) sleep through most of their expected duration -- the SHORTEST of the site's last eight waits
    // at this batch size (a phase has a floor and outliers are always longer: one 10 ms hiccup must not make the next waits
    // oversleep), only phases above 250 us -- and spin only for the last 30 %: a spinning wait keeps a core busy for the whole GPU phase,
    // and an 8-GPU node has few cores per rank (wait_event, kosk_ctx.cpp).  Measured with nine callers in three cohorts: the same
    // throughput (148-151 k proofs/s either way) at 3.5 busy cores fewer together with KOSK_POOL_SPIN_US=0 (profiles/r05_sweep_host.txt)
    bool wait_nap = true;
    bool blocking_sync = false; // kosk_options::blocking_sync: every host wait sleeps on an event instead of spinning (few host cores per GPU)
    int xof_max_blocks = 32;    // KOSK_DEBUG_XOF_BLOCKS=n lowers gen_matrix's block limit (tests force the error path with 1)
    // strict_encoding (kosk_options::strict_encoding; DEFAULT 1 since round 6): the verifier marks a proof malformed
    // (fail bit 0) when ANY u16 element of a record the reference reads is >= q -- no honest prover emits one, and accepting them makes
    // proofs malleable (v and v + q verify alike).  0 = the reference-following mode of round 5: such elements are treated exactly as
    // the reference treats them, record by record: folded where it only multiplies / converts to ZZ_p, raw in its
    // non-reducing add / sub and comparisons; pinned against the oracle by two differential suites, opt-in for parity work
    bool strict_encoding = true;
    // Fiat-Shamir aggregation on the device (kosk_options::fs_mode = KOSK_FS_DEVICE): the four
    // sha3_256 chains of a prove + verify over the 46.5 KB digest tables run as one wave per proof where the tables are, the challenge
    // vectors / opened lists / the verifier's I' == I never leave HBM, and the resident calls have NO host round trip left: no digest
    // table crosses PCIe, the host neither hashes nor waits between segments (kosk_fs_kernels.hip).  Host mode (default)
    // is the path of rounds 1-5
    bool fs_device = false;
    bool host_register = true;       // KOSK_REGISTER=0: staging copies only, even for buffers the caller page-locked itself.  (KOSK_REGISTER=2 of
                                     // rounds 2-4 -- the library page-locking PAGEABLE caller memory for a call -- is gone: both process aborts on
                                     // record happened inside calls that had just done that, and neither was ever reproduced or explained)
};

// Per-proof buffers: B records each, allocated by ctx_create and ensure_verify_workspace with INV_PER_PROOF.  Pointers only
struct CtxBlock {
    uint16_t *d_P = nullptr;
    uint8_t *d_tape = nullptr, *d_dig1 = nullptr, *d_dig2 = nullptr, *d_proof = nullptr;
    // seeded proving: the seeds of a call, 32 bytes per proof (page-locked staging and its device copy, which k_tape_expand reads)
    uint8_t *d_seedbuf = nullptr, *h_seedbuf = nullptr;
    int16_t *d_A = nullptr, *d_se = nullptr;
    // key generation on the device (kosk_keygen_kernels.hip)
    // one record per proof [pk | NTT(s) bytes | sha3_512 output], kg_rec bytes apart, so that the key generation's
    // outputs cross PCIe in ONE copy; d_pk / d_sb / d_seeds (and the h_ mirrors) point into it, all with stride kg_rec
    uint8_t *d_kg = nullptr, *h_kg = nullptr;
    uint8_t *d_seeds = nullptr, *d_pk = nullptr, *d_sb = nullptr; // sha3_512 output, packed pk, packed NTT(s)
    uint8_t *h_seeds = nullptr, *h_pk = nullptr, *h_sb = nullptr;
    int16_t *d_sehat = nullptr;
    uint16_t *d_t = nullptr; // pk's t, canonical (verifier)
    uint16_t *d_alpha = nullptr, *d_I = nullptr, *d_rest = nullptr; // d_rest / h_rest: the second half of d_I's / h_I's allocation (one upload)
    int32_t *d_pwT = nullptr;
    uint8_t *d_coef = nullptr; // K3 operand: alpha-power coefficients as a limb matrix
    uint32_t *d_fail = nullptr;      // [proof] bit mask of failed checks (FailBit)
    // d_bind / h_bind: the call's binding values (kosk-bind-v1, CtxPrivate::bind_ctx), written by k_bind_values in BOTH Fiat-Shamir modes;
    // in host mode they cross PCIe with the first digest table
    uint8_t *d_bind = nullptr, *h_bind = nullptr;
    // pinned host staging
    uint8_t *h_tape = nullptr, *h_dig = nullptr, *h_dig2 = nullptr, *h_proof = nullptr; // h_dig / h_dig2: the host's copies of the two digest tables
    uint16_t *h_alpha = nullptr, *h_I = nullptr, *h_rest = nullptr;
    uint32_t *h_fail = nullptr;
    // verifier workspace (allocated on first use, kosk_verify.cpp)
    uint16_t *d_O = nullptr;         // opened matrix [proof][nrows][OS] (kosk_params.hpp)
    uint16_t *d_w = nullptr, *d_ell = nullptr;
    int16_t *d_node_of = nullptr;
    uint16_t *d_isort = nullptr, *d_hrange = nullptr;
    uint8_t *d_gather = nullptr, *d_gather2 = nullptr; // weighted shares as MFMA fragment tiles (k_gather_frags)
    uint16_t *d_sec = nullptr, *d_sec_u1 = nullptr, *d_sec_u2 = nullptr;
    uint16_t *h_Iimg = nullptr;      // I fields as read from the proof images
    // The verifier's host needs both digest tables whole (mlwe_verifier.cpp:40-44, :648-652), but only 150 entries per proof and
    // round are NEW -- the rest are fields of the proof image.  When the caller handed the proofs over in host memory (host_img:
    // kosk_verify_batch) the host reads those 1304 digests per table straight from the caller's images, only the 150 recomputed ones per
    // proof follow each round's hash (4.8 KB instead of 46.5 KB on the critical path), and the host puts the table together
    // (assemble_digest_table).  For resident proofs the whole tables are copied behind each hash (the split with early copies on a
    // side stream measured slower and is gone since round 6: profiles/r04_digest_paths.txt).
    uint8_t *d_odig = nullptr, *h_odig = nullptr; // [proof][NOPEN][32] recomputed digests of the opened parties (one round at a time)
};

struct CtxPrivate {
    // the buffer inventory: owns every buffer this context allocated, lists a view's windows (kosk_inventory.hpp)
    Inventory inv;
    int max_batch = 0;
    // Inventory::add through the HIP error check (KOSK_HIPCHK(c.own(...))): allocate, record and own in one line
    template <class T>
    hipError_t own(const char *name, T **at, size_t bytes, int flags, int group = Inventory::INVG_CORE, size_t sec_off = 0, size_t sec_bytes = (size_t)-1,
                   size_t alloc_bytes = 0)
    {
        return (hipError_t)inv.add(name, at, bytes, flags, group, sec_off, sec_bytes, alloc_bytes);
    }
    // kosk_wipe_secrets cleared staged prover inputs: kosk_prove_resident refuses until a staging call has run again
    bool staged_wiped = false;
    bool is_view = false;
    int view_first = 0;
    int own_batch = 0;   // proofs of this context's own callers (a view: its member's kosk_create size; else max_batch)
    // the largest batch ONE call may run on this context: own_batch, except while this view leads a merged run of its cohort
    // (kosk_capi.cpp: RunScope raises it to the run's total).  A view's max_batch is everything behind its first proof in the
    // arena -- its neighbours' blocks included -- so no entry point may size a chunk by max_batch
    int call_cap = 0;
    int reserved_threads = 1; // workers the pool was created with (a call never creates threads: nthreads <= this)
    int nthreads = 1;
    Pool *pool = nullptr; // this context's host worker threads
    std::string err;
    randombytes_fn rb = nullptr;
    void *rb_user = nullptr;
    // kosk_set_entropy: what a call with tapes == NULL draws through `rb` -- false (default) the reference's 64 / M x 32 / 302-byte
    // sequence, a whole tape per proof; true ONE 32-byte seed per proof, expanded on the device
    bool entropy_seed = false;
    round_fn round_hook = nullptr;
    void *round_user = nullptr;

    // the tapes the kernels read: d_tape after an upload, or the caller's own device buffer used in place
    const uint8_t *tape_cur = nullptr;
    size_t tape_cur_stride = 0;
    TapeSegs tape_segs{}; // a merged call whose callers' device tapes are read in place (count > 0; valid for that call only)
    int resident_pk_n = 0; // pk records valid in d_pk (written by the key generation or a verifier staging call): pk_mode 2 needs >= n
    // kosk_kem_enc_verified encapsulates to d_pk with the bits of a verify call that read d_A / d_t: it must know that d_A / d_t were decoded
    // from d_pk (keys_from_pk_n: how many leading records of d_A / d_t are decodings of the same records of d_pk; 0 once instances were
    // uploaded, kosk_split.cpp) and that neither changed since (pk_epoch counts every change of either).  EVERY writer of d_pk goes through
    // note_pk_written(), the instance upload through note_keys_from_inst(), a verify call that decodes the resident d_pk again
    // (pk_mode 2) through note_pk_decoded()
    unsigned long pk_epoch = 0;
    int keys_from_pk_n = 0;
    void note_pk_written(int n) { resident_pk_n = n; keys_from_pk_n = n; pk_epoch++; }
    void note_pk_decoded(int n) { if (n > keys_from_pk_n) keys_from_pk_n = n; } // records [0, n) decoded again from d_pk; the others keep their state
    void note_keys_from_inst() { keys_from_pk_n = 0; pk_epoch++; }
    const uint8_t *host_img = nullptr;            // the caller's host copy of the proof images of THIS call (kosk_verify_batch; CtxBlock::d_odig)
    size_t host_img_stride = 0;
    hipEvent_t ev = nullptr;
    std::vector<uint16_t> v_I2, v_rest2; // the verifier's recomputed opened lists (kept across calls: two fresh 0.4 MB vectors per call were
                                         // an mmap, a page fault per page and a munmap on the tail of every verify call)
    std::function<void()> near_end_hook; // set by a merged run's executor: called once when only the call's tail is left (kosk_combine.hpp: near_end)
    bool kg_on_host_pending = false; // ev_kg was recorded by this call's key generation
    hipEvent_t ev_kg = nullptr; // the key records (pk, NTT(s) bytes, seeds) of a keygen-in-front call are on the host once it has passed
    // the histories behind CtxShared::wait_nap
    enum { WAIT_SITES = 8 };
    enum { WAIT_HIST = 8 };
    // (round 6) a site keeps WAIT_SIZES histories, one per batch size it has recently seen (a cohort whose merged runs alternate
    // between two sizes -- 276 and 230 proofs when one member is late -- no longer forgets what it learnt at every change), least
    // recently used first out
    enum { WAIT_SIZES = 2 };
    struct WaitHist {
        int n = 0;                    // batch size this history belongs to (0: unused)
        int at = 0;                   // next entry to overwrite
        unsigned long stamp = 0;      // last use (for the replacement)
        double us[WAIT_HIST] = {0};   // the last measured waits (0 = empty): the nap is sized by their MINIMUM
    };
    WaitHist wait_hist[WAIT_SITES][WAIT_SIZES];
    unsigned long wait_stamp = 0;
    hipEvent_t ev_sync = nullptr; // what a blocking_sync / napping wait sleeps on
    hipEvent_t timer_ev[2] = {nullptr, nullptr}; // kosk_stream_timer_start / _stop
    // compact wire format staging (allocated on first use)
    CompactPlan cplan{};
    size_t compact_stride = 0;
    uint8_t *d_compact = nullptr, *h_compact = nullptr;
    uint32_t *d_compact_bad = nullptr, *h_compact_bad = nullptr;
    // dense wire format: its field plan and record stride in the compact staging buffers; the refill's workspace (allocated on first use)
    CompactPlan dplan{};
    size_t dense_stride = 0;
    CompactPlan d2plan{}; // kosk-dense-v2
    size_t dense2_stride = 0;
    uint16_t *d_dense_ws = nullptr;
    uint32_t *d_dense_status = nullptr;
    TcWs *tc = nullptr; // kosk_transcode_batch: allocated at this context's first such call, owned by it like `kem`

    // device-raised errors (XofGuard): one word of page-locked host memory the kernels store to; checked and cleared by
    // device_error_check() after a call's last synchronisation (a view's kernels report to the view's own word)
    uint32_t *h_err = nullptr;

    // hipGraph per pipeline segment (the launches between two host Fiat-Shamir rounds), captured once per
    // batch size and replayed: one API call instead of ~15 launches of kernels that run 3-6 us each.
    enum SegId { SEG_P1 = 0, SEG_P1B, SEG_P2, SEG_P2B, SEG_P3, SEG_V1, SEG_V1B, SEG_V2, SEG_V2B, SEG_COUNT };
    struct SegGraph {
        hipGraphExec_t exec = nullptr;
        int n = 0;
        // caller-owned pointers baked into the captured launches (SEG_P1: the tape buffer read in place): part of the cache key
        const void *key_ptr = nullptr;
        size_t key_stride = 0;
    };
    SegGraph seg[SEG_COUNT];
    bool use_graphs = false; // KOSK_GRAPHS=1 turns them on (measured on ROCm 7.2: no gain over plain launches)
    bool capturing = false;
    // kosk-bind-v1 (kosk_set_contexts): while bind_n > 0 the context is ARMED -- prove_resident and verify_resident hash
    // B_b = k_bind_values(pk_b, context_b) behind both digest tables of proof b.  bind_ctx: the handle's device copy of the armed contexts,
    // 32 bytes each (owned by the handle, kosk_capi.cpp); bind_first: the position in the caller's whole call of this call's proof 0
    // (set by the entry point for every chunk / sub-batch).  The call's binding values: CtxBlock::d_bind / h_bind
    const uint8_t *bind_ctx = nullptr;
    int bind_n = 0, bind_first = 0;
    // tests (kosk_force_opened_candidates): while force_n > 0 round 2 of prove_resident takes the candidates of proof b from list
    // bind_first + b -- force_d in HBM for the chain kernel, force_h for the host's round; both owned by the handle (kosk_capi.cpp).  The
    // verifier never looks at them
    const uint16_t *force_d = nullptr, *force_h = nullptr;
    int force_n = 0;
    // which of the library's paths really ran on this context (kosk_path_count): the tests of the knobs assert on these
    long path_n[PATH_COUNT] = {0};
    KemWs *kem = nullptr; // allocated at this context's first KEM call, owned by it (a view's is its own, never the arena's)
    KemKey *kem_key = nullptr; // the key slot: allocated at the first kem_key_set, its own allocation (kem_ensure never moves it), owned like `kem`
    KemRegistry *registry = nullptr; // the verified-key registry: allocated by registry_reserve, its own allocations, owned like `kem`
    KemRegistry *monitor = nullptr;  // the registry monitor (kosk_monitor.hip): allocated by monitor_reserve, owned like `registry`
    // the relying party's staging (kosk_relying.hip): one launch group of peer data, allocated at the first checking call and
    // grown like the KEM workspace; public entries of the inventory under INVG_RELYING
    uint8_t *d_rl_rec = nullptr;   // [rl_cap][rl_rec] the paths (depth x 32) or the proof records of the items
    uint8_t *d_rl_q = nullptr;     // [rl_cap][32] the claimed fingerprints h / the query fingerprints x
    uint8_t *d_rl_state = nullptr; // [rl_cap] the claims "occupied" / "empty"
    uint8_t *d_rl_ok = nullptr;    // [rl_cap] the verdicts
    int32_t *d_rl_slot = nullptr;  // [rl_cap] the claimed slots
    int rl_cap = 0;
    size_t rl_rec = 0;
    // the head signer (kosk_headsig.hip): allocated by headsig_signer_reserve on a handle with a history, freed with the
    // history or the registry; entries of the inventory under INVG_SIGNER, the seed a secret one and long-lived like the resident KEM key
    int sg_height = 0;             // 0: no signer
    bool sg_has_seed = false;      // false after wipe_secrets(): the tree and the public key stay, signing is refused
    uint8_t *d_sg_tree = nullptr;  // [headsig::tree_bytes(sg_height)] T[r] at 32 r
    uint8_t *d_sg_seed = nullptr;  // [64] the seed; behind it a candidate seed while a reserve checks it against the standing tree, else zeros
    uint8_t *d_sg_sig = nullptr;   // [headsig::sig_bytes(sg_height) + 32] one staged signature, the signed root behind it
    uint8_t sg_pub[52] = {0};

    double phase_sec[PH_COUNT] = {0};
    int prof_on = 0; // 1: the graded kernel only (graphs stay on); 2: every profiled id (plain launches)
    hipEvent_t prof_ev[PR_COUNT][2] = {};
    bool prof_used[PR_COUNT] = {};
    double prof_ms[PR_COUNT] = {0};
    long prof_n[PR_COUNT] = {0};
    long prof_units[PR_COUNT] = {0}; // proofs served by the timed launches (a merged run serves several callers' batches per launch)
    int prof_cur_units[PR_COUNT] = {0};

    // witness recovery (witness_from_sk): the secret-key records of the largest call so far and their verdicts; allocated at the first
    // such call and owned by this context like `kem`
    int wit_cap = 0;
    uint8_t *d_wsk = nullptr, *d_wok = nullptr, *h_wok = nullptr;
    uint8_t *d_wsalt = nullptr; // kosk-keyseed-v1: the call's salts, 32 bytes per key (allocated with d_wsk)

    // the offline bank (kosk_bank.hip): bank_cap entries of bank_entry_bytes(P) each in one allocation of this context's
    // own, made by bank_reserve() and nowhere else.  A FIFO ring: the oldest of the bank_ready entries lies in slot bank_head, a fill appends
    // behind the youngest.  A free slot is all zero (k_bank_take zeroes what it reads; a fill that fails behind its put zeroes the slots it wrote)
    uint8_t *d_bank = nullptr;
    int bank_cap = 0, bank_ready = 0, bank_head = 0;
    // the last staging call took the offline rows from the bank (stage_prover_keys_banked): the next prove_resident runs the online front
    // only, and is the only one -- it ends with no staged inputs, as a banked key generation does, because the tape buffer never held the
    // offline sections of these proofs and the rows of a consumed entry serve one proof.  Every call that makes other tapes current clears it
    bool staged_online = false;
};

struct Ctx : CtxShared, CtxBlock, CtxPrivate {
    Ctx();
    ~Ctx(); // graph execs, events, the workers; every buffer through the inventory; the stream unless this is a view
    XofGuard xof_guard() const { XofGuard g; g.err = h_err; g.max_blocks = xof_max_blocks; return g; }
    void prof_begin(int id, int units = 0) { if (prof_on && !capturing) { (void)hipEventRecord(prof_ev[id][0], stream); prof_cur_units[id] = units; } }
    void prof_end(int id) { if (prof_on && !capturing) { (void)hipEventRecord(prof_ev[id][1], stream); prof_used[id] = true; } }
    void prof_collect(); // call after the stream has been synchronised
};

// Run `body` (stream launches on c.stream only: kernels, pinned-memory copies, memsets) as segment `seg`:
// captured into a graph on first use for this batch size, replayed afterwards.
template <class F>
int run_segment(Ctx &c, int seg, int n, F &&body, const void *key_ptr = nullptr, size_t key_stride = 0)
{
    if (seg < 0 || !c.use_graphs || c.prof_on == 2) return body();
    Ctx::SegGraph &g = c.seg[seg];
    if (g.exec && (g.n != n || g.key_ptr != key_ptr || g.key_stride != key_stride)) {
        (void)hipGraphExecDestroy(g.exec);
        g.exec = nullptr;
    }
    if (!g.exec) {
        hipError_t e = hipStreamBeginCapture(c.stream, hipStreamCaptureModeThreadLocal);
        if (e != hipSuccess) { c.err = std::string("hipStreamBeginCapture: ") + hipGetErrorString(e); return -1; }
        c.capturing = true;
        int rc;
        try {
            rc = body();
        } catch (...) { // never leave the stream in capture mode (the handle would be unusable afterwards)
            c.capturing = false;
            hipGraph_t dead = nullptr;
            (void)hipStreamEndCapture(c.stream, &dead);
            if (dead) (void)hipGraphDestroy(dead);
            throw;
        }
        c.capturing = false;
        hipGraph_t graph = nullptr;
        e = hipStreamEndCapture(c.stream, &graph);
        if (rc) {
            if (graph) (void)hipGraphDestroy(graph);
            return rc;
        }
        if (e != hipSuccess || !graph) { c.err = std::string("hipStreamEndCapture: ") + hipGetErrorString(e); return -1; }
        e = hipGraphInstantiate(&g.exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (e != hipSuccess) { g.exec = nullptr; c.err = std::string("hipGraphInstantiate: ") + hipGetErrorString(e); return -1; }
        g.n = n;
        g.key_ptr = key_ptr;
        g.key_stride = key_stride;
    }
    const hipError_t e = hipGraphLaunch(g.exec, c.stream);
    if (e != hipSuccess) { c.err = std::string("hipGraphLaunch: ") + hipGetErrorString(e); return -1; }
    c.path_n[PATH_GRAPH_REPLAY]++;
    return 0;
}

// what kosk_create_ex's options struct decides per context (-1 / 0 = not given: the default; no environment variable is consulted)
struct CtxOpts {
    int host_threads = 0;    // kosk_options::host_threads
    int blocking_sync = -1;  // kosk_options::blocking_sync
    int strict_encoding = -1; // kosk_options::strict_encoding
    int fs_device = -1;      // kosk_options::fs_mode == KOSK_FS_DEVICE
};
// host_share: sub-contexts of the same handle that share this process's CPUs (divides the host thread budget)
int ctx_create(Ctx **out, int device, int kyber_k, int max_batch, std::string &err, int host_share = 1, const CtxOpts &opts = CtxOpts());
// a view of `arena` starting at proof `first` whose own callers send up to `own_batch` proofs per call; reserve_threads: host
// workers created now (a merged run led by this view uses base_threads x members of them)
int ctx_make_view(Ctx &arena, int first, int own_batch, int reserve_threads, Ctx **out, std::string &err);

// p is device memory (hipMalloc); plain, page-locked and unknown pointers are host memory
bool is_device_pointer(const void *p);
// host wait for everything queued on the context's stream (spinning, or sleeping with kosk_options::blocking_sync)
hipError_t stream_sync(Ctx &c);
// wait for `ev` (recorded on the context's stream); site = which of the pipeline's long waits this is (0..WAIT_SITES-1: napped with
// KOSK_WAIT_NAP=1), n = the batch size the wait belongs to; site < 0: a plain wait
hipError_t wait_event(Ctx &c, hipEvent_t ev, int site, int n);
hipError_t stream_sync_site(Ctx &c, int site, int n);
// a round's digest table of n proofs from HBM into the context's page-locked host memory, on the context's stream (the caller records c.ev behind it)
hipError_t copy_round_table(Ctx &c, uint8_t *h_dst, const uint8_t *d_src, int n);
// a small copy between HBM and one of the library's OWN page-locked host buffers, rows x row_bytes (kernel or hipMemcpy[2D]Async)
hipError_t copy_small(Ctx &c, void *dst, size_t dst_stride, const void *src, size_t src_stride, size_t row_bytes, size_t nrows, hipMemcpyKind kind, hipStream_t st);
// after the stream has been synchronised: -1 (with c.err set, the word cleared) if a kernel of this context raised an error
int device_error_check(Ctx &c);
// armed context (bind_n > 0): -1 with c.err set if the call's n proofs reach behind the armed contexts, else the binding values of the
// n public keys resident in d_pk are queued on the stream (k_bind_values -> d_bind; host Fiat-Shamir: and copied to h_bind).  0 otherwise
int bind_check(Ctx &c, int n);
int issue_bind_values(Ctx &c, int n);
// C[g][rows_d[i]][off + m] = sum_k T[m][k] * src[g][rows_s[i]][koff + k] mod q on the table kernels; -1 (c.err set) if the operands
// fail table_gemm_ok() (kosk_device.hpp: 16-byte aligned source and output rows), which nothing the library itself issues does
int gemm_modq(Ctx &c, const GemmTable &t, const GemmSrc &s, const GemmDst &d, int npg, int ngroups);

// tapes (host or device memory, nullptr = callback) -> pk/sk on host, tape + key material resident in HBM
// seeds != nullptr: seeded proving, the tapes are expanded on the device from 32-byte seeds (host or device memory) and `tapes` is not read
int stage_prover_inputs(Ctx &c, int n, const uint8_t *tapes, size_t tape_stride, uint8_t *pk, uint8_t *sk, const uint8_t *seeds = nullptr,
                        size_t seed_stride = 0);
// n seeds (host or device memory) -> n tapes in DEVICE memory (base and stride multiples of 8), on the context's stream, synchronised
int tape_expand_device(Ctx &c, int n, const uint8_t *seeds, size_t seed_stride, uint8_t *d_tapes, size_t tape_stride);
// draw n 32-byte seeds through the context's randombytes callback / OS entropy, one call per proof, in proof order
void draw_seeds(const Ctx &c, int n, uint8_t *out);
// its three parts: make the tapes resident (async), kyber_keygen on the device + D2H of pk / NTT(s) / seeds (async),
// and, once the stream has been synchronised, the host half (sk = NTT(s) || pk || H(pk) || z, kosk.cpp:62-69)
int upload_tapes(Ctx &c, int n, const uint8_t *tapes, size_t tape_stride);
int issue_keygen(Ctx &c, int n, bool sampled = false);
void finish_keygen_host(Ctx &c, int n, uint8_t *pk, uint8_t *sk);
// Existing keys (kosk_witness_kernels.hip): n <= call_cap secret-key records (host or device memory) -> A, s, e and the embedded pk bytes
// resident exactly as a key generation leaves them (d_A, d_t, d_se, d_pk; note_pk_written), s and e all zero where ok[b] = 0 (a
// coefficient outside [-eta1, eta1]).  se_out (host, may be nullptr): n x 2 K x 256 int16, s then e.  Synchronised.
int witness_from_sk(Ctx &c, int n, const uint8_t *sk, int16_t *se_out, uint8_t *ok);
void witness_release(Ctx &c);
// the counterpart of stage_prover_inputs for such keys: tapes (exactly one of tapes / seeds / derived; the first 64 bytes of a tape, the
// key generation's seed, are not read) + witness resident for prove_resident.
// derived (kosk-keyseed-v1): the seeds come from the records themselves, k_keyseed -> d_seedbuf -> k_tape_expand; an
// armed context hashes the armed contexts bind_first .. bind_first + n (set by the entry point, as for prove_resident), salts (host or
// device memory, nullptr: the deterministic form) are salt_stride >= 32 apart
struct DerivedSrc {
    const uint8_t *salts = nullptr;
    size_t salt_stride = 0;
};
int stage_prover_keys(Ctx &c, int n, const uint8_t *sk, const uint8_t *tapes, size_t tape_stride, const uint8_t *seeds, size_t seed_stride, uint8_t *ok,
                      const DerivedSrc *derived = nullptr);
// kernel level: n seeds of format kosk-keyseed-v1 into DEVICE memory (8-byte aligned), every input host or device memory; synchronised
int keyseed_device(Ctx &c, int n, const uint8_t *sk, const uint8_t *contexts, size_t context_stride, const uint8_t *salts, size_t salt_stride, uint8_t *d_seeds);
// everything from resident inputs to resident proof images (two host Fiat-Shamir round trips)
// FRONT_OFFLINE: FRONT_RANDOMNESS and FRONT_RANGE in one pass (one launch of each kernel), what a bank entry is made by
enum FrontPart { FRONT_FULL = 0, FRONT_RANDOMNESS, FRONT_RANGE, FRONT_ONLINE, FRONT_OFFLINE };
int issue_sharing_front(Ctx &c, int n, FrontPart part, bool with_keygen = false);
// online_only: the offline material (f, NTT f, eta sharings) is already in the row matrix (prove_prepared, the banked calls; implied
// after stage_prover_keys_banked, which the call uses up: a second prove_resident needs a new staging call; so does one after a banked key
// generation).  An armed context binds as usual: the pk bytes must be resident (prove_prepared has none and refuses)
// keygen != nullptr: key generation runs at the head of the first segment (no extra synchronisation) and pk / sk are
// written before the call returns -- the whole kyber_verifiable_keygen, proofs left resident
int prove_resident(Ctx &c, int n, bool online_only = false, const KeygenIn *keygen = nullptr);
// the reference's second-level entry points on host structs (kosk_split.cpp); struct layouts in include/kosk_mi355x.h
size_t randomness_bytes(const Params &P);
size_t range_proof_bytes(const Params &P);
size_t mlwe_inst_bytes(const Params &P);
int prepare_randomness(Ctx &c, int n, const uint8_t *tapes, size_t tape_stride, uint8_t *rand_out);
int prepare_range_proof(Ctx &c, int n, const uint8_t *tapes, size_t tape_stride, uint8_t *range_out);
int prove_prepared(Ctx &c, int n, const uint8_t *inst, const uint8_t *rand_in, const uint8_t *range_in, const uint8_t *tapes,
                   size_t tape_stride, uint8_t *pi);
int stage_verifier_inst(Ctx &c, int n, const uint8_t *pi, const uint8_t *inst);
// ---- the offline bank (kosk_bank.hip) ----
// the three sections of a tape: 0 key seed [0, 64), 1 offline [64, O), 2 online [O, T)
enum { TAPE_SEC_KEYSEED = 0, TAPE_SEC_OFFLINE = 1, TAPE_SEC_ONLINE = 2 };
inline bool tape_section(const Params &P, int section, size_t *offset, size_t *size)
{
    const size_t O = 64 + (size_t)32 * P.M + (size_t)302 * (2 * P.M + 2 * P.K * P.E);
    const size_t lo[4] = {0, 64, O, P.tape_bytes};
    if (section < 0 || section > 2) return false;
    *offset = lo[section];
    *size = lo[section + 1] - lo[section];
    return true;
}
// sections `mask` (bit s = section s) of n tapes made current for the fronts that read exactly those: explicit tapes (host memory: only
// the sections cross PCIe; device memory: read in place when aligned, else the sections are copied) or seeds (kosk-seedtape-v1, expanded
// on the device).  Exactly one of tapes / seeds.  compact (host memory only): a record holds exactly the sections of `mask` back to back
// instead of a whole tape (what the entry points draw when they are given neither).  Queued on the stream, not synchronised
int stage_tape_sections(Ctx &c, int n, unsigned mask, const uint8_t *tapes, size_t tape_stride, const uint8_t *seeds, size_t seed_stride, bool compact = false);
inline size_t bank_entry_bytes(const Params &P) { return (size_t)(2 * P.M + 2 * P.K * P.E) * RS * sizeof(uint16_t); } // whole rows, RS columns each
// capacity 0 wipes and frees; a non-empty bank is refused.  The old allocation is wiped before it is freed
int bank_reserve(Ctx &c, int capacity);
void bank_release(Ctx &c); // frees without wiping (the destructor: kosk_destroy has wiped)
void bank_note_wiped(Ctx &c); // wipe_secrets() zeroed the bank: it is empty
// n <= call_cap entries appended in proof order: the offline front on the given tapes / seeds, then k_bank_put; bank_ready + n <= bank_cap
// is the caller's check.  Synchronised; staged prover inputs are gone afterwards (the tape buffer was reused)
int bank_fill(Ctx &c, int n, const uint8_t *tapes, size_t tape_stride, const uint8_t *seeds, size_t seed_stride, bool compact = false);
// the n oldest entries into the row matrix of proofs 0..n-1 (k_bank_take: the slots are zero afterwards); n <= bank_ready is the caller's
// check.  The entries are gone once this has been called, whatever it returns.  Queued on the stream, not synchronised
int bank_take(Ctx &c, int n);
// stage_prover_keys for a banked proof: the online section of the tapes / seeds, the witness of the records, the n oldest entries of the
// bank; prove_resident(c, n) then runs online-only.  Ends with the stream synchronised up to the witness
int stage_prover_keys_banked(Ctx &c, int n, const uint8_t *sk, const uint8_t *tapes, size_t tape_stride, const uint8_t *seeds, size_t seed_stride, uint8_t *ok,
                             bool compact = false);
// diagnostic (tools/bank_rate.py): `reps` times k_bank_put + k_bank_take of n entries on scratch slots, and the runtime's own copies and
// fill of the same bytes, each between two events
int bank_timing(Ctx &c, int n, int reps, double *put_ms, double *take_ms, double *copy_ms, double *copy_fill_ms, size_t *bytes);
int ensure_verify_workspace(Ctx &c);
// ---- wire formats: the image, and the three packed forms of it (kosk_compact.hip; kosk_dense.hip: v1 and v2) ----
enum { FMT_IMAGE = 0, FMT_COMPACT = 1, FMT_DENSE = 2, FMT_DENSE2 = 4 }; // KOSK_FMT_* (kosk_capi.cpp asserts the equality); 3 is no format
inline bool fmt_dense(int fmt) { return fmt == FMT_DENSE || fmt == FMT_DENSE2; } // a format with dropped rows: refill behind unpack, codeword check before pack
// what one format is on a context: its field plan (nullptr: the image), the bytes of a record on the wire and its stride in HBM / staging
struct WireFmt {
    int id;
    const CompactPlan *plan;
    size_t bytes, stride;
};
void ensure_plans(Ctx &c); // cplan, dplan, d2plan and their strides (no buffer); wire_fmt() of a packed format needs it
inline WireFmt wire_fmt(const Ctx &c, int fmt)
{
    if (fmt == FMT_IMAGE) return WireFmt{fmt, nullptr, c.P.proof_bytes, c.image_stride};
    if (fmt == FMT_DENSE2) return WireFmt{fmt, &c.d2plan, c.d2plan.bytes, c.dense2_stride};
    return fmt == FMT_DENSE ? WireFmt{fmt, &c.dplan, c.dplan.bytes, c.dense_stride} : WireFmt{fmt, &c.cplan, c.cplan.bytes, c.compact_stride};
}
size_t format_bytes(const Params &P, int fmt); // of one record; 0 for an unknown format
// n resident images <-> n records of format `fmt` in host memory; direct: the host buffer is page-locked (copied to / from straight, no
// staging).  The image bodies (kosk_ctx.cpp, kosk_verify.cpp) and the packed ones (kosk_compact.hip: pack in front of the D2H copy, unpack
// and for dense the refill behind the H2D copy) differ on purpose: call_cap against own_batch (packed calls are never merged), the staging
// buffers, the PH_D2H clock
int fetch_proofs_image(Ctx &c, int n, uint8_t *pi, bool direct = false);
int fetch_proofs_packed(Ctx &c, int n, int fmt, uint8_t *out, bool direct = false);
int stage_verifier_inputs_image(Ctx &c, int n, const uint8_t *pi, const uint8_t *pk, bool direct = false);
int stage_verifier_inputs_packed(Ctx &c, int n, int fmt, const uint8_t *in, const uint8_t *pk, bool direct = false);
inline int fetch_proofs(Ctx &c, int n, int fmt, uint8_t *out, bool direct = false)
{
    return fmt == FMT_IMAGE ? fetch_proofs_image(c, n, out, direct) : fetch_proofs_packed(c, n, fmt, out, direct);
}
inline int stage_verifier_inputs(Ctx &c, int n, int fmt, const uint8_t *in, const uint8_t *pk, bool direct = false)
{
    return fmt == FMT_IMAGE ? stage_verifier_inputs_image(c, n, in, pk, direct) : stage_verifier_inputs_packed(c, n, fmt, in, pk, direct);
}
int ensure_dense_ws(Ctx &c);
// check = true: the codeword check (k_dense_check): the refill compared with the images' own rows 407..1303 instead of stored, the images only read
// (the pointer is not const because the fill shares the signature); d_status 0, 1 malformed I, 2 a dropped row that is not the refill
// fmt: FMT_DENSE or FMT_DENSE2 (its own kernels, dropped rows and counters)
int dense_fill_launch(Ctx &c, int n, uint8_t *d_images, size_t image_stride, uint32_t *d_status, bool check = false, int fmt = FMT_DENSE); // n <= own_batch, on c.stream, not synchronised
int dense_fill_device(Ctx &c, int n, uint8_t *d_images, size_t image_stride, uint32_t *d_status, bool check = false, int fmt = FMT_DENSE);
// transcoding between the wire formats (kosk_compact.hip): n <= own_batch records, `in` / `out` host or device memory of any alignment,
// status[b] (host) the host codecs' composition (kosk_mi355x.h); touches nothing but its own workspace and the refill's scratch.  Synchronised
int transcode(Ctx &c, int n, int from, const uint8_t *in, int to, uint8_t *out, int32_t *status);
void transcode_release(Ctx &c);
// pk_mode 0: A and t are already resident (stage_verifier_inputs / stage_verifier_inst); 1: decode `pk` (host or
// device memory, n records of pk_bytes) at the head of the first segment (kosk.cpp:94-99: polyvec_frombytes + gen_matrix);
// 2: decode the pk bytes the key generation left resident in HBM
int verify_resident(Ctx &c, int n, uint8_t *ok, int pk_mode = 0, const uint8_t *pk = nullptr, const VerifySeg *segs = nullptr);

// Kyber KEM (kosk_kem_kernels.hip): n <= KEM_CHUNK items, every buffer host or device memory, unmerged on the context's stream.
// crypto_kem_enc_derand (kem.c:76-96): pk == nullptr encapsulates to the public keys resident in c.d_pk from record resident_first on; mask (host, n bytes, or
// nullptr): items whose byte is 0 are not encapsulated to, their ct and ss are zero-filled.  crypto_kem_dec (kem.c:140-169).
int kem_enc(Ctx &c, int n, const uint8_t *pk, const uint8_t *coins, uint8_t *ct, uint8_t *ss, const uint8_t *mask = nullptr, int resident_first = 0);
int kem_dec(Ctx &c, int n, const uint8_t *ct, const uint8_t *sk, uint8_t *ss);
// crypto_kem_keypair_derand (kem.c:25-35): coins n x 64 bytes, d || z.  Touches the KEM workspace only: not pk_epoch, not the resident keys.
int kem_keypair(Ctx &c, int n, const uint8_t *coins, uint8_t *pk, uint8_t *sk);
// FIPS 203 7.2 / 7.3 input checks on n pk (is_sk = 0) or sk records: flags[b] = OR of KOSK_KEYCHK_* (kosk_mi355x.h)
enum { KEYCHK_HASH = 1, KEYCHK_PK_RANGE = 2, KEYCHK_S_RANGE = 4 }; // KOSK_KEYCHK_* (kosk_capi.cpp asserts the equality)
int kem_check(Ctx &c, int n, const uint8_t *rec, int is_sk, uint8_t *flags);
void kem_release(Ctx &c);
// One resident key.  kem_key_set: exactly one of pk / sk, one record, host or device memory; replaces the slot (the old one
// is wiped first); synchronised; -1 ("block limit") leaves the slot empty.  kem_enc_key / kem_dec_key: n <= KEM_CHUNK items on the slot's
// key, per-item work only; kem_dec_key needs state KEM_KEY_SK and refuses a wiped slot.  kem_key_clear wipes and frees the slot.
enum { KEM_KEY_NONE = 0, KEM_KEY_PK = 1, KEM_KEY_SK = 2 }; // KOSK_KEM_KEY_* (kosk_capi.cpp asserts the equality)
int kem_key_set(Ctx &c, const uint8_t *pk, const uint8_t *sk);
int kem_key_state(const Ctx &c);
int kem_key_clear(Ctx &c);
void kem_key_release(Ctx &c); // frees without wiping (the destructor: kosk_destroy has wiped)
void kem_key_note_wiped(Ctx &c); // wipe_secrets() zeroed the slot's secret part: SK -> PK
int kem_enc_key(Ctx &c, int n, const uint8_t *coins, uint8_t *ct, uint8_t *ss);
int kem_dec_key(Ctx &c, int n, const uint8_t *ct, uint8_t *ss);

// The verified-key registry (kosk_registry.hip): `capacity` slots in HBM, structure of arrays -- what depends on a key alone, decoded
// once at admission (k_registry_admit) and read by kem_enc_slots through KemKeySide, slot s at base + s * stride.  Four allocations of its
// own (kem_ensure frees and reallocates the KEM workspace; the registry must not move) and a fifth, the fingerprint index, from the first
// lookup on: public buffers of the inventory under INVG_REGISTRY.
// `occ` mirrors d_flag on the host: every mutation goes through a host call.
struct KemRegistry {
    int capacity = 0, used = 0;
    uint8_t *d_pk = nullptr;   // [capacity][384 K + 32] the pk bytes as admitted
    uint8_t *d_h = nullptr;    // [capacity][32]         SHA3-256 of those bytes
    int16_t *d_A = nullptr;    // [capacity][K K][256]   A^T, the layout encrypt_block reads
    uint8_t *d_flag = nullptr; // [capacity]             1 = occupied
    std::vector<uint8_t> occ;
    // the fingerprint index: allocated at the first call that looks a key up, rebuilt by that call when a mutation cleared
    // index_valid
    int32_t *d_index = nullptr; // [registry_index_entries(capacity)] -1 = empty, else the lowest occupied slot of one fingerprint
    bool index_valid = false;
    // the registry tree (kosk-regtree-v1): allocated at the first tree call, brought up to date by the first tree call after
    // a mutation -- tier 0 over the leaf subtrees (1 024 slots each) that a mutation marked, every upper tier whole
    uint8_t *d_tree = nullptr;   // [regtree::tree_bytes(capacity)] every node of every level, level-major
    int32_t *d_dirty = nullptr;  // [regtree::subtrees(D)] the subtree numbers of one tier-0 launch: block i hashes subtree d_dirty[i]
    uint8_t *d_paths = nullptr;  // [paths_cap] staging of k_registry_path's sibling records for one launch group
    size_t paths_cap = 0;
    bool tree_valid = false;
    std::vector<uint8_t> dirty;  // [subtrees] 1 = a slot of the leaf subtree changed since the tree was current; empty while there is no tree
    // a mutation wrote or zeroed `slot`
    void tree_touch(size_t slot)
    {
        tree_valid = false;
        if (!dirty.empty()) dirty[slot >> 10] = 1;
    }
    // the sorted tree (kosk-regsort-v1): allocated at the first call of kosk_registry_sorted_root / _prove_absent, rebuilt whole
    // by the first such call after a mutation cleared sorted_valid (wherever index_valid is cleared)
    uint8_t *d_srec = nullptr;   // [P][16] the sort records, ascending: the first `used` name the occupied slots in (fingerprint, slot) order
    uint8_t *d_stree = nullptr;  // [regtree::tree_bytes(capacity)] every node of every level, level-major
    uint8_t *d_sq = nullptr;     // [sproof_cap][32] the staged queries of one launch group
    int32_t *d_srank = nullptr;  // [sproof_cap][2] per query: lb, present
    uint8_t *d_skind = nullptr;  // [sproof_cap] per query: 1 absent, 2 present
    uint8_t *d_sproof = nullptr; // [sproof_cap][regsort::proof_bytes(D)] the staged proof records
    int sproof_cap = 0;
    bool sorted_valid = false;
    // a mutation changed the set of occupied slots or a fingerprint
    void lookups_stale() { index_valid = false; sorted_valid = false; }
    // the history (kosk-reghist-v1): allocated by kosk_registry_history_reserve, appended to by every mutating call from then
    // on; a registry without one (hist_max == 0) allocates and launches what it did before
    int hist_max = 0, hist_size = 0;
    uint8_t *d_hev = nullptr;    // [hist_max][80] the stored event records
    uint8_t *d_hnode = nullptr;  // [reghist::nodes_bytes(hist_max)] the complete nodes, level-major; a node is written once
    uint8_t *d_hrag = nullptr;   // [33][32] R_l of hist_frontier: the ragged nodes, the root at bit_length(size)
    int32_t *d_hjob = nullptr;   // [KEM_CHUNK][2] (op, slot) of one append launch
    int32_t *d_hq = nullptr;     // [hstage_cap] the staged indices / old sizes of one launch group
    uint8_t *d_hleaf = nullptr;  // [hstage_cap][32] the staged leaves
    uint8_t *d_hproof = nullptr; // [hstage_cap][reghist::consistency_bytes(hist_max)] the staged proof records
    int hstage_cap = 0;
    int hist_frontier = -1;      // the size d_hrag belongs to; -1: none yet
    // the monitor (kosk_monitor.hip) is a registry of fingerprints and flags alone (d_pk == d_A == nullptr, no mirror, no
    // event records) whose buffers come and go with INVG_MONITOR; the tree, sorted-tree and history functions below take either
    int inv_group = Inventory::INVG_REGISTRY;
    bool mon_failed = false;     // a feed was rejected: the state is that of events [0, hist_size) until the monitor is reserved again
    uint8_t *d_mstage = nullptr; // [KEM_CHUNK][80] the stored records of one launch group, 16-byte aligned
    uint8_t *d_mrec = nullptr;   // [KEM_CHUNK][16] the sort records of one segment
    uint32_t *d_mword = nullptr; // [0] the verdict: (index << 8) | reason of the lowest invalid event, MONITOR_WORD_OK while there is none; [1] used
    // the inventory name of a buffer: "registry.<field>" or "monitor.<field>"
    const char *buf_name(const char *registry_name, const char *monitor_name) const { return inv_group == Inventory::INVG_REGISTRY ? registry_name : monitor_name; }
};
inline size_t registry_slot_bytes(int K) { return (size_t)384 * K + 32 + 32 + (size_t)K * K * 512 + 1; }
// One launch of k_registry_admit: key b of n (16-byte aligned records in HBM, `src_stride` apart, a multiple of 16) into slot[b] (device
// memory; < 0: masked, nothing is written).  wave: K^2 + 1 one-wave blocks per key; else one sponge per lane.  Queued, not synchronised
struct RegAdmitJob {
    int n, K, pk_bytes, wave;
    const uint8_t *src;
    size_t src_stride;
    const int32_t *slot;
    uint8_t *pk, *h, *flag;
    int16_t *A;
    uint32_t *err;
    int max_blocks;
};
hipError_t launch_registry_admit(const RegAdmitJob &j, hipStream_t st);
// capacity 0 frees; a non-empty registry is refused; -1 leaves nothing allocated
int registry_reserve(Ctx &c, int capacity);
void registry_release(Ctx &c);
// the named slots' records and flags zeroed (k_wipe), the mirror updated; slots are valid ids, repeats allowed; synchronised
int registry_evict(Ctx &c, int n, const int32_t *slots);
// state (host), pk / h (host or device memory, or nullptr) of the named slots; an empty slot reads as zeros; synchronised
int registry_read(Ctx &c, int n, const int32_t *slots, uint8_t *state, uint8_t *pk, uint8_t *h);
// n <= KEM_CHUNK keys into slots[b] (host; valid and distinct ids, or < 0: masked): pk records in host or device memory, or pk == nullptr: the
// keys resident in c.d_pk from record resident_first on.  Synchronised; -1 ("block limit") with the mirror untouched -- the caller evicts
int kem_registry_admit(Ctx &c, int n, const uint8_t *pk, int resident_first, const int32_t *slots);
// crypto_kem_enc_derand for n <= KEM_CHUNK items, item b to the key in slots[b] (host; valid ids): per-item work only; an empty slot's ct and ss
// are zero-filled
int kem_enc_slots(Ctx &c, int n, const int32_t *slots, const uint8_t *coins, uint8_t *ct, uint8_t *ss);

// The fingerprint index (kosk_registry.hip): open addressing over the slots' H(pk), T = the smallest power of two >= 2 x capacity
// int32 entries, linear probing from LE32(h[0..4)) & (T - 1); one entry per distinct fingerprint among the occupied slots, holding the
// lowest such slot.
inline size_t registry_index_entries(int capacity)
{
    if (capacity < 1) return 0;
    size_t t = 2;
    while (t < 2 * (size_t)capacity) t <<= 1;
    return t;
}
inline uint32_t registry_index_home(int capacity, const uint8_t *h)
{
    const uint32_t w = (uint32_t)h[0] | (uint32_t)h[1] << 8 | (uint32_t)h[2] << 16 | (uint32_t)h[3] << 24;
    return w & (uint32_t)(registry_index_entries(capacity) - 1);
}
// k_registry_index: one lane per slot, the table memset to -1 in front of it
struct RegIndexJob {
    int capacity;
    uint32_t mask;       // T - 1
    const uint8_t *h;    // [capacity][32]
    const uint8_t *flag; // [capacity]
    int32_t *index;      // [T]
    uint32_t *err;
};
// k_registry_find: one lane per query (q: [n][32], 16-byte aligned).  slot (may be nullptr): the slot or -1; key / mask (both or neither):
// what the KEM kernels read, the slot or 0 on a miss, and 1 / 0
struct RegFindJob {
    int n, capacity;
    uint32_t mask;
    const uint8_t *q, *h;
    const int32_t *index;
    int32_t *slot, *key;
    uint8_t *found;
    uint32_t *err;
};
hipError_t launch_registry_index(const RegIndexJob &j, hipStream_t st);
hipError_t launch_registry_find(const RegFindJob &j, hipStream_t st);
// the index allocated and current: a no-op while index_valid; else memset + k_registry_index, synchronised; -1 ("index overflow")
int registry_index_ensure(Ctx &c);
// n <= KEM_CHUNK fingerprints (n x 32 bytes, host or device memory of any alignment) -> slots (n int32, host or device memory): the lowest
// occupied slot with that H(pk), or -1.  Synchronised; the staged fingerprints are zeroed
int kem_registry_find(Ctx &c, int n, const uint8_t *h, int32_t *slots);
// the first half of an enrolment: H(pk) of n <= KEM_CHUNK candidates (as kem_registry_admit names them) into h (host, n x 32) and what
// k_registry_find says of them into hit (host).  Synchronised; the staged records and fingerprints are zeroed
int kem_registry_probe(Ctx &c, int n, const uint8_t *pk, int resident_first, uint8_t *h, int32_t *hit);
// crypto_kem_enc_derand for n <= KEM_CHUNK items, item b to the key whose H(pk) is h[b] (host or device memory): k_registry_find writes the
// slot index and the mask in HBM, the per-item kernels follow; done (host or device memory) = found, ct and ss of a miss zero-filled
int kem_enc_peers(Ctx &c, int n, const uint8_t *h, const uint8_t *coins, uint8_t *ct, uint8_t *ss, uint8_t *done);

// The registry tree (kosk_registry.hip, kosk_regtree.hpp).
// k_registry_tree, one tier: block i reduces up to 1 024 inputs through up to 10 levels in LDS and writes every node to the tree.  Tier 0
// forms the leaves from flag / h (positions >= capacity and empty slots are `empty`) and takes its subtree number from list[i]; an upper
// tier reads level 10 tier of the tree and block i is subtree i
enum { REGTREE_WAVE_TAIL = 8 }; // levels of this many nodes or fewer run one wave per node on the wave sponge
struct RegTreeJob {
    int tier, D, K, capacity, wave_tail;
    const uint8_t *h, *flag;
    const int32_t *list;
    uint64_t empty[4]; // E as words
    uint8_t *tree;
};
// k_registry_path: per item b the D sibling records of slot[b] (level l: node (slot >> l) ^ 1), zeros where slot[b] < 0, into paths[b][D][32];
// hout (may be nullptr): the slot's stored fingerprint, zeros for slot < 0; found (may be nullptr): slot >= 0
struct RegPathJob {
    int n, D;
    const int32_t *slot;
    const uint8_t *tree, *h;
    uint8_t *paths, *hout, *found;
};
hipError_t launch_registry_tree(const RegTreeJob &j, unsigned blocks, hipStream_t st);
hipError_t launch_registry_path(const RegPathJob &j, hipStream_t st);
// the tree allocated and current: a no-op while tree_valid; else the tiers, synchronised
int registry_tree_ensure(Ctx &c, KemRegistry &r);
inline int registry_tree_ensure(Ctx &c) { return registry_tree_ensure(c, *c.registry); }
// r.d_paths holds n items' paths
int registry_paths_ensure(Ctx &c, int n);
// the root of the current tree to `root` (host or device memory); synchronised
int registry_root(Ctx &c, KemRegistry &r, uint8_t *root);
inline int registry_root(Ctx &c, uint8_t *root) { return registry_root(c, *c.registry, root); }
// n <= KEM_CHUNK paths.  slots != nullptr (host; valid ids): of those slots, with their stored fingerprints to hout (or nullptr); else of the
// lowest occupied slots that hold the fingerprints h (k_registry_find in front), with those slots to slots_out and found to done.  paths (may
// be nullptr when D = 0), hout, slots_out, done: host or device memory.  Synchronised; what was staged in the KEM workspace is zeroed
int kem_registry_prove(Ctx &c, int n, const int32_t *slots, const uint8_t *h, uint8_t *hout, int32_t *slots_out, uint8_t *done, uint8_t *paths);

// The sorted tree (kosk_regsort.hip, kosk_regsort.hpp).
// A sort record is 16 bytes: the first 8 bytes of the fingerprint as a big-endian number (two words, low first), the slot, the class (0: an
// occupied slot; 1: an empty slot or padding, which sorts last).  The order is (class, prefix, bytes 8..31 of h[slot] where two class-0
// prefixes tie, slot).  regsort_sort: a bitonic network over 2^lg records -- tiles of 2^REGSORT_TILE_LG records in LDS (k_regsort_tile),
// compare-exchange steps at a distance of a tile or more in HBM (k_regsort_step).  Queued, not synchronised; every launch counts in
// PATH_REGSORT_SORT
// 2 048 records, 32 KB of LDS (the residency of k_registry_tree), one compare-exchange per lane and step: measured against tiles of 2^10
// and 2^12 records and blocks of 256 and 512 threads
enum { REGSORT_TILE_LG = 11, REGSORT_TILE_THREADS = 1024 };
struct RegSortJob {
    int n, lg;           // records < n come from flag / h, the rest up to 2^lg are padding
    int phase, jg;       // k_regsort_tile: the merge phase it finishes (0: every phase up to the tile); k_regsort_step: phase and distance, as logarithms
    const uint8_t *h, *flag;
    uint8_t *rec;
    int32_t *order;      // k_regsort_order: record i < n to its slot, or -1 for class 1
};
int regsort_sort(Ctx &c, const RegSortJob &j);
// the network alone, over records that are in place (k_monitor_keys wrote them): what regsort_sort runs behind k_regsort_keys
int regsort_network(Ctx &c, const RegSortJob &j);
// k_regsort_tree, one tier, the shape of k_registry_tree: tier 0 forms S(h[slot], slot) from record i < used and Z from there on
struct RegSortTreeJob {
    int tier, D, K, used;
    const uint8_t *h, *rec;
    uint64_t pad[4]; // Z as words
    uint8_t *tree;
};
// k_regsort_rank: one lane per query, lb and present by binary search; k_regsort_prove: one lane per 16-byte piece of a proof record
struct RegSortProveJob {
    int n, D, used;
    const uint8_t *q, *h, *rec, *tree;
    int32_t *rank;
    uint8_t *kind, *proof;
};
// the sorted tree allocated and current: a no-op while sorted_valid; else keys, sort, tiers, synchronised
int registry_sorted_ensure(Ctx &c, KemRegistry &r);
inline int registry_sorted_ensure(Ctx &c) { return registry_sorted_ensure(c, *c.registry); }
// the root of the current sorted tree to `root` (host or device memory); synchronised
int registry_sorted_root(Ctx &c, KemRegistry &r, uint8_t *root);
inline int registry_sorted_root(Ctx &c, uint8_t *root) { return registry_sorted_root(c, *c.registry, root); }
// n <= KEM_CHUNK queries (host or device memory of any alignment) -> kind[b] and one proof record each.  Synchronised; the staged queries
// are zeroed
int registry_prove_absent(Ctx &c, int n, const uint8_t *h, uint8_t *kind, uint8_t *records);
// the sort alone on caller-made fingerprints and flags in device memory (h 8-byte aligned): d_order[i] = the index of the i-th entry, -1 from
// the number of flagged records on.  Synchronised; the records live in a buffer that comes and goes with the call
int regsort_order_device(Ctx &c, int n, const uint8_t *d_h, const uint8_t *d_flag, int32_t *d_order);

// The history (kosk_reghist.hip, kosk_reghist.hpp).
// k_reghist_append, one tier: block i owns group (s >> 10 tier >> 10) + i of 1 024 inputs of level 10 tier.  Tier 0 writes the records of
// events [s, s + c) (from job[e - s] = (op, slot) and h[slot], or, where job is nullptr, the one checkpoint from root_a / root_b / used /
// capacity), hashes their leaves and loads the older ones; an upper tier loads its inputs.  Then up to 10 levels through LDS: a node is
// hashed and written iff it became complete, (i + 1) 2^l in (s, s + c], and loaded otherwise
struct RegHistAppendJob {
    int tier, D, K, s, c; // D: reghist::depth(hist_max), the layout of `nodes`
    const int32_t *job;
    const uint8_t *h, *root_a, *root_b;
    uint32_t used, capacity;
    uint8_t *ev, *nodes;
    const uint8_t *rec; // k_monitor_leaves: the stored records of events [s, s + c), 16-byte aligned
};
// k_reghist_frontier: one wave; rag[l + 1] = R_(l + 1) of size n for every l, the fold of the complete subtrees of the set bits of n up to l
struct RegHistFrontierJob {
    int D, n;
    const uint8_t *nodes;
    uint8_t *rag;
};
// k_reghist_prove: a lane pair per query.  kind 0: the inclusion record of leaf q[b] at `size` (and that leaf to leaves, may be nullptr);
// kind 1: the consistency record from q[b] to `size`.  rec_bytes per record, header, nodes, zero padding
struct RegHistProveJob {
    int n, kind, D, size, rec_bytes;
    const int32_t *q;
    const uint8_t *nodes, *rag;
    uint8_t *leaves, *proof;
};
// max_events 0 frees; -1 (c.err set) leaves the earlier state
int reghist_reserve(Ctx &c, int max_events);
// `count` events (op[i], slot[i]) read against the CURRENT d_h; the caller has checked that they fit.  Queued and synchronised
int reghist_append(Ctx &c, int count, const int32_t *ops, const int32_t *slots);
int reghist_checkpoint(Ctx &c, int *index);
// the root at size (<= hist_size) to `root` (host or device memory)
int reghist_head(Ctx &c, KemRegistry &r, int size, uint8_t *root);
inline int reghist_head(Ctx &c, int size, uint8_t *root) { return reghist_head(c, *c.registry, size, root); }
// the tiers of one append of cnt events to r's history of s events.  j.rec != nullptr: tier 0 is k_monitor_leaves over those stored records;
// else j.job names the events, or (j.job == nullptr) j carries the operands of one checkpoint.  Queued, not synchronised
int reghist_append_launch(Ctx &c, KemRegistry &r, RegHistAppendJob j, int s, int cnt);
int reghist_read(Ctx &c, int first, int n, uint8_t *events);
// n <= KEM_CHUNK queries (host, validated) at `size`; leaves (kind 0) and records: host or device memory, leaves may be nullptr
int reghist_prove(Ctx &c, int kind, int size, int n, const int32_t *q, uint8_t *leaves, uint8_t *records);

// The registry monitor (kosk_monitor.hip): the replay of a stored event log onto a table of fingerprints and
// flags, with every checkpoint's roots, used and capacity compared in HBM.
enum { MONITOR_OK = 0, MONITOR_BAD_RECORD = 1, MONITOR_BAD_SLOT = 2, MONITOR_ADMIT_OCCUPIED = 3, MONITOR_EVICT_EMPTY = 4, MONITOR_EVICT_MISMATCH = 5,
       MONITOR_CP_USED = 6, MONITOR_CP_CAPACITY = 7, MONITOR_CP_SLOT_ROOT = 8, MONITOR_CP_SORTED_ROOT = 9 };
enum : uint32_t { MONITOR_WORD_OK = 0xFFFFFFFFu };
// One segment: n staged records (ev, 80 bytes each, 16-byte aligned) of absolute indices base .. base + n - 1.
// k_monitor_keys: the record check and the 16-byte sort records (prefix = (slot << 32) | position, class 0; an invalid record and the
// positions from n to 2^lg are class 1).  k_monitor_apply over the sorted records: commit == 0 checks the ADMIT / EVICT rule against the
// previous event of the same slot or the table and writes nothing to the table; commit == 1 returns at once where word[0] is set, else
// writes every touched slot's final flag and fingerprint and adds the net change of `used` to word[1]
struct MonitorJob {
    int n, lg, base, capacity, commit;
    const uint8_t *ev;
    uint8_t *rec, *h, *flag;
    uint32_t *word;
};
// k_monitor_check, one wave: the staged checkpoint record against word[1], capacity and the two root nodes; the verdict to word[0]
struct MonitorCheckJob {
    int index, capacity;
    const uint8_t *ev, *root_a, *root_b;
    uint32_t *word;
};
hipError_t launch_monitor_keys(const MonitorJob &j, hipStream_t st);
hipError_t launch_monitor_apply(const MonitorJob &j, hipStream_t st);
hipError_t launch_monitor_check(const MonitorCheckJob &j, hipStream_t st);
hipError_t launch_monitor_leaves(const RegHistAppendJob &j, unsigned blocks, hipStream_t st);
// (0, 0) frees; any other pair starts a fresh, empty replay; -1 (c.err set) leaves no monitor
int monitor_reserve(Ctx &c, int capacity, int max_events);
void monitor_release(Ctx &c);
// the next n events (host or device memory of any alignment; the caller has checked that they fit): 1 accepted, 0 rejected with the lowest
// invalid index and its lowest reason, -1 an error
int monitor_feed(Ctx &c, int n, const uint8_t *events, int *bad_index, int *reason);
int monitor_roots(Ctx &c, uint8_t *slot_root, uint8_t *sorted_root);
// registry_read without the pk: the flags are read from HBM (a monitor keeps no mirror)
int monitor_read(Ctx &c, int n, const int32_t *slots, uint8_t *state, uint8_t *h);

// The relying party (kosk_relying.hip): proofs of the two state trees checked in batches against one root.
// k_regtree_check: one lane per item; ok[b] = 1 iff slot[b] lies in [0, 2^D) and the walk of kosk_regtree.hpp from L(h_b) (state == nullptr
// or state[b] != 0; a claim "occupied" without fingerprints, h == nullptr, gives 0) or E up paths[b][D][32] ends in root.  h_b lies at
// h + b * h_stride (8-byte aligned), paths 16-byte aligned
struct RegTreeCheckJob {
    int n, D, K;
    const int32_t *slot;
    const uint8_t *state, *h;
    size_t h_stride;
    const uint8_t *paths;
    uint64_t root[4];
    uint8_t *ok;
};
// k_regsort_check: a lane pair per item, one walk each; verdict[b] = regsort::check_proof(K, D, x_b, rec_b, root).  x and the records
// (regsort::proof_bytes(D) apart) 16-byte aligned
struct RegSortCheckJob {
    int n, D, K;
    const uint8_t *x, *rec;
    uint64_t root[4];
    uint8_t *verdict;
};
hipError_t launch_regtree_check(const RegTreeCheckJob &j, hipStream_t st);
hipError_t launch_regsort_check(const RegSortCheckJob &j, hipStream_t st);
// the staging holds n items with records of rec_bytes each (n rounded up to 1 024, at most KEM_CHUNK): all five buffers or none
int relying_ensure(Ctx &c, int n, size_t rec_bytes);
// n <= KEM_CHUNK items, every array host or device memory of any alignment (state, h: may be nullptr; paths: where D == 0), root: host.
// Synchronised; touches nothing but the staging
int regtree_check_paths(Ctx &c, int n, int D, const int32_t *slots, const uint8_t *state, const uint8_t *h, const uint8_t *paths, const uint8_t *root, uint8_t *ok);
int regsort_check_proofs(Ctx &c, int n, int D, const uint8_t *x, const uint8_t *records, const uint8_t *root, uint8_t *verdict);
// crypto_kem_enc_derand for n <= KEM_CHUNK items, item b to pk_b iff (slots[b], occupied, SHA3-256(pk_b), paths_b) walks to root: H(pk) into
// the KEM workspace, k_regtree_check writes the mask in HBM, the per-item kernels follow (kosk_kem_kernels.hip); done = the verdicts, ct and
// ss of a failed item zero-filled
int kem_enc_proven(Ctx &c, int n, int D, const uint8_t *pk, const int32_t *slots, const uint8_t *paths, const uint8_t *root, const uint8_t *coins,
                   uint8_t *ct, uint8_t *ss, uint8_t *done);

// Signed heads (kosk_headsig.hip, kosk_headsig.hpp).
// k_headsig_leaves: a lane per (leaf, chain), 7 leaves a block; leaf first + i of `count` to tree (T[2^h + q] at 32 (2^h + q)), or, where out
// is not nullptr, to out + 32 i
struct HeadSigLeavesJob {
    int h;
    uint32_t first, count;
    uint64_t id[2];
    const uint8_t *seed;
    uint8_t *tree, *out;
};
// k_headsig_tree, one tier: block i reduces up to 1 024 nodes of level 10 tier (counted from the leaves) through up to 10 levels in LDS
struct HeadSigTreeJob {
    int h, tier;
    uint64_t id[2];
    uint8_t *tree;
};
// k_headsig_sign: one block; the root of `size` is read at root (HBM) or, where root is nullptr, is root_imm; the record to sig, the root
// behind it
struct HeadSigSignJob {
    int h, K;
    uint32_t size;
    uint64_t id[2], root_imm[4];
    const uint8_t *seed, *root, *tree;
    uint8_t *sig;
};
// k_headsig_verify: a lane per (item, chain), 7 items a block; ok[b] = headsig::verify(pub, K, roots_b, sizes[b], sigs_b) == 1.  roots and
// the records (sig_bytes apart) 16-byte aligned
struct HeadSigVerifyJob {
    int n, h, K;
    uint64_t id[2], top[4];
    const uint8_t *roots, *sigs;
    const int32_t *sizes;
    size_t sig_bytes;
    uint8_t *ok;
};
// height 0 frees (the seed is wiped first).  Needs c.registry with a history; seed, id, pub: host or device memory.  The same (height, id)
// over a standing tree whose leaf 0 the seed reproduces restores the seed and builds nothing.  Synchronised
int headsig_signer_reserve(Ctx &c, int height, const uint8_t *seed, const uint8_t *id, uint8_t *pub);
void headsig_signer_release(Ctx &c);
void headsig_note_wiped(Ctx &c); // wipe_secrets() zeroed the seed
// the head of `size` (validated: a size of the history, below 2^height) signed with leaf `size`; sig, root: host or device memory
int headsig_sign_head(Ctx &c, int size, uint8_t *sig, uint8_t *root);
// n <= KEM_CHUNK items against one public key (host, its height validated); every array host or device memory of any alignment
int headsig_verify_heads(Ctx &c, int n, const uint8_t *pub, const uint8_t *roots, const int32_t *sizes, const uint8_t *sigs, uint8_t *ok);
// d_hrag holds the ragged nodes and the root of `size` >= 1: queued, not synchronised (kosk_reghist.hip)
int reghist_frontier_ensure(Ctx &c, KemRegistry &r, int size);

// ---- erasure (kosk_wipe.hip) ----
enum { WIPE_MAX_REGIONS = 48 }; // regions per launch of k_wipe (they travel in the kernel arguments); longer lists take more launches
enum : unsigned long long { WIPE_MEMSET_BYTES = 320ull << 20 }; // a single run of this many bytes or more is cleared by hipMemsetAsync (kosk_wipe.hip)
// zero the regions: queued on the context's stream (never while it is capturing), not synchronised; empty regions are skipped
int launch_wipe(Ctx &c, const WipeRegion *regions, int n);
// zero every secret buffer of the inventory, HBM by k_wipe and page-locked staging by the host; synchronised.  A view wipes its own block
// of the per-proof buffers and its private buffers.  Staged prover inputs are gone afterwards (staged_wiped).  keep_key (the wipe at the end
// of a call under KOSK_WIPE_CALL): the resident KEM key and the unconsumed entries of the offline bank are long-lived secrets, not per-call
// scratch, and stay
int wipe_secrets(Ctx &c, bool keep_key = false);
// the HBM regions wipe_secrets() clears (group >= 0: of that owner only; skip_mask: bit g set = not owner g's)
int wipe_regions_list(const Ctx &c, std::vector<WipeRegion> &out, int group = -1, unsigned skip_mask = 0);
// the secret HBM buffers of one owner (Inventory::INVG_*), synchronised: before they are freed to be allocated larger
int wipe_group(Ctx &c, int group);
void host_wipe(void *p, size_t bytes); // explicit_bzero: not removed as a dead store
template <class T> void host_wipe_vec(std::vector<T> &v) { if (!v.empty()) host_wipe(v.data(), v.size() * sizeof(T)); }
// a host heap temporary that carries secrets is cleared before it is freed, however its scope ends
template <class T> struct VecWiper {
    std::vector<T> &v;
    explicit VecWiper(std::vector<T> &v_) : v(v_) {}
    ~VecWiper() { host_wipe_vec(v); }
    VecWiper(const VecWiper &) = delete;
    VecWiper &operator=(const VecWiper &) = delete;
};
// occurrences of needle[0, len) at every byte offset of every buffer of the inventory, secret or public, HBM (k_scan) and page-locked host
// memory; d_needle / d_slots / h_slots: the caller's scratch (kosk_capi.cpp).  Synchronised
int secret_scan(Ctx &c, const uint8_t *needle, size_t len, const uint8_t *d_needle, unsigned long long *d_slots, unsigned long long *h_slots, long *hits);
enum { SCAN_SLOT_COUNT = 1024 };

} // namespace kosk
