// extern "C" boundary (include/kosk_mi355x.h) over kosk::Ctx.
//
// Containment rules of this file (the reference's API is void / bool and never kills its caller except on RNG failure,
// kosk.hpp:18-24, kyber/randombytes.c:49-52):
//   * no C++ exception leaves an extern "C" function: every entry point runs inside guard(), which turns std::exception /
//     anything else into rc -1 + kosk_last_error() text;
//   * no thread is created inside a batch call: the S - 1 lane threads of a handle (KOSK_STREAMS = S) and every
//     sub-context's host workers are created by kosk_create(), whose failure is an ordinary -1;
//   * the library never page-locks caller memory (round 5: KOSK_REGISTER=2, which did for the duration of a multi-chunk call, is
//     gone -- both process aborts on record happened inside calls that had just done so and neither was ever explained);
//     buffers the caller page-locked itself (kosk_host_alloc, hipHostMalloc, hipHostRegister) are copied to / from directly,
//     everything else goes through the library's own pinned staging buffers.
#include "../../include/kosk_mi355x.h"

#include <unistd.h>

#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <exception>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "kosk_combine.hpp"
#include "kosk_ctx.hpp"
#include "kosk_lanes.hpp"
#include "kosk_registry_resolve.hpp"
#include "kosk_headsig.hpp"
#include "kosk_reghist.hpp"
#include "kosk_regsort.hpp"
#include "kosk_regtree.hpp"

using namespace kosk;

struct kosk_ctx;
// A cohort (KOSK_COMBINE = C): up to C handles of equal (device, kyber_k, max_batch) are views of ONE arena context, and their
// resident calls are served by merged pipeline runs (kosk_combine.hpp)
struct Cohort {
    int device = 0, k = 0, per = 0;
    CtxOpts opts; // what the members' options asked of the shared context: a handle only joins a cohort created with the same
    Ctx *arena = nullptr;
    std::unique_ptr<Combiner> comb;
    std::vector<kosk_ctx *> member;
};
static std::mutex g_cohort_mu; // creation / destruction of cohorts and their members
static std::vector<Cohort *> g_cohorts;
enum CombineKind { CK_ALONE = -1, CK_KEYGEN = 0, CK_VERIFY_PK_GIVEN = 1, CK_VERIFY_PK_RESIDENT = 2 };

// A handle owns S sub-contexts (own stream + HBM workspace each).  A batch call splits its proofs into S
// contiguous sub-batches that run concurrently on S host threads: while one sub-batch sits in a host
// Fiat-Shamir round trip the GPU works on the other, and kernels of different streams share the CUs.
struct kosk_ctx {
    std::vector<Ctx *> sub;
    LaneSet lanes; // lane i runs sub[i]; lane 0 is the caller's thread (kosk_lanes.hpp)
    Ctx *c = nullptr; // sub[0]: kernel-level entry points, error text, sizes
    int max_batch = 0;
    std::string err;
    std::vector<uint32_t> masks; // fail masks of the last verify call, in the caller's proof order
    int masks_n = 0;             // proofs of the last verify call (kosk_verify_fail_masks serves exactly these)
    Cohort *cohort = nullptr;    // KOSK_COMBINE: this handle is member `member_i` of a cohort, sub[0] a view of its arena
    int member_i = -1;
    long merged_calls = 0, merged_members = 0; // resident calls of this handle served by a run, and the members those runs served
    // kosk_kem_enc_verified: the last completed verify call left its public keys in HBM (pk_epoch of sub[0] at that moment), whole
    // (one pipeline run, not chunks that overwrote each other) -- verify_keys 0: no such call, 1: yes, 2: chunked, 3: no pk bytes (instances)
    unsigned long verify_epoch = 0;
    int verify_keys = 0;
    bool hooks_unmerged = false; // kosk_options::hooks_unmerged: with a round hook set, this handle's resident calls run on their own
    // kosk_set_contexts (kosk-bind-v1): the handle's own copy of the armed contexts in HBM, 32 bytes each; every sub-context points at it
    uint8_t *d_contexts = nullptr;
    int armed = 0;
    int wipe_mode = 0; // kosk_set_wipe: KOSK_WIPE_CALL ends every secret-bearing entry point with wipe_secrets() on every sub-context
    void disarm()
    {
        for (Ctx *x : sub) { x->bind_ctx = nullptr; x->bind_n = 0; x->bind_first = 0; }
        if (c) c->inv.release(Inventory::INVG_BIND); // frees d_contexts, which sub[0]'s inventory owns
        armed = 0;
    }
    // kosk_force_opened_candidates (tests): the handle's lists, 150 candidates each, in HBM for the chain kernel and on the host for the
    // host's round; every sub-context points at both
    uint16_t *d_force = nullptr;
    std::vector<uint16_t> h_force;
    void unforce()
    {
        for (Ctx *x : sub) { x->force_d = nullptr; x->force_h = nullptr; x->force_n = 0; }
        if (c) c->inv.release(Inventory::INVG_FORCE); // frees d_force likewise
        h_force.clear();
    }

    ~kosk_ctx()
    {
        lanes.lanes.clear(); // join the lane threads before their sub-contexts go
        // nothing secret goes back to the allocator readable: every sub-context (a cohort member: its own block and private buffers)
        for (Ctx *x : sub) {
            try { (void)wipe_secrets(*x); } catch (...) {}
        }
        disarm();
        unforce();
        for (Ctx *x : sub) delete x;
        if (cohort) {
            std::lock_guard<std::mutex> lk(g_cohort_mu);
            cohort->member[member_i] = nullptr;
            if (const char *e = getenv("KOSK_COMBINE_TRACE"))
                if (atoi(e)) fprintf(stderr, "[kosk combine] cohort %p %s\n", (void *)cohort, cohort->comb->trace(member_i).c_str());
            if (cohort->comb->leave(member_i) == 0) { // the last member wipes the whole arena and frees it
                try { (void)wipe_secrets(*cohort->arena); } catch (...) {}
                delete cohort->arena;
                g_cohorts.erase(std::remove(g_cohorts.begin(), g_cohorts.end(), cohort), g_cohorts.end());
                delete cohort;
            }
        }
    }
    // every entry point starts from a clean error state (kosk_last_error never reports a stale message)
    void clear_err()
    {
        err.clear();
        for (Ctx *x : sub) x->err.clear();
    }
    int run_lanes(std::vector<std::function<int()>> &jobs)
    {
        std::vector<int> rc;
        std::vector<std::string> what;
        lanes.run(jobs, rc, what);
        if (rc.size() < sub.size() || what.size() < sub.size()) { // no memory even for the bookkeeping: nothing was started
            err = "out of memory while dealing a batch call to the handle's lanes";
            c->err = err;
            return -1;
        }
        for (int i = 0; i < (int)sub.size(); i++)
            if (rc[i]) {
                if (rc[i] == -2) sub[i]->err = "exception in a batch job: " + what[i];
                err = sub[i]->err;
                c->err = err;
                return -1;
            }
        return 0;
    }
    // an n-proof call (n <= max_batch) as S contiguous sub-batches: fn(sub-context, first, count)
    template <typename F>
    int run(int n, F &&fn)
    {
        clear_err();
        auto on_lane = [&](int i, int first, int count) { return fn(*sub[i], first, count); };
        std::vector<std::function<int()>> jobs;
        deal_split((int)sub.size(), n, on_lane, jobs);
        return run_lanes(jobs);
    }
};

// Every extern "C" entry point's body runs in here: nothing thrown below (std::bad_alloc, std::system_error, an exception
// out of a host worker job) reaches the caller's frames.
template <typename F>
static int guard(kosk_ctx *ctx, const char *fn, F &&body) noexcept
{
    try {
        // a stale per-thread HIP error (an earlier failed call of ours, or of the host application) must not be taken for
        // the result of this call's first kernel launch: the launchers report hipGetLastError().  Documented in the header:
        // every entry point RESETS the calling thread's HIP last-error state, so the application has to look at the outcome of
        // its own launches before it calls in here
        (void)hipGetLastError();
        return body();
    } catch (const std::exception &e) {
        try {
            if (ctx) { ctx->err = std::string(fn) + ": " + e.what(); if (ctx->c) ctx->c->err = ctx->err; }
        } catch (...) {}
    } catch (...) {
        try {
            if (ctx) { ctx->err = std::string(fn) + ": unknown exception"; if (ctx->c) ctx->c->err = ctx->err; }
        } catch (...) {}
    }
    return -1;
}
template <typename F>
static int guard(const kosk_ctx *, const char *, F &&body) noexcept // read-only entry points leave the error string alone
{
    try {
        return body();
    } catch (...) {
    }
    return -1;
}
#define GUARD(ctx) return guard(ctx, __func__, [&]() -> int {
#define GUARD_END });

// KOSK_WIPE_CALL (kosk_set_wipe): an entry point that brings secrets onto the handle ends with the wipe of every sub-context, however its
// body ends -- success, an error return, an exception.  Mode off: one untaken branch
static int wipe_handle(kosk_ctx *h, bool keep_key = false)
{
    int rc = 0;
    for (Ctx *x : h->sub)
        if (wipe_secrets(*x, keep_key)) { h->err = x->err; h->c->err = x->err; rc = -1; }
    return rc;
}
template <typename F>
static int wiped_call(kosk_ctx *h, F &&body)
{
    if (!h->wipe_mode) return body();
    int rc;
    try {
        rc = body();
    } catch (...) {
        try { (void)wipe_handle(h, true); } catch (...) {}
        throw;
    }
    if (wipe_handle(h, true) && !rc) rc = -1; // the resident KEM key is a long-lived secret, not per-call scratch: it stays
    return rc;
}
#define WGUARD(ctx) return guard(ctx, __func__, [&]() -> int { return wiped_call(ctx, [&]() -> int {
#define WGUARD_END }); });

// The one way a call is refused with a message: it has done nothing, and kosk_last_error(ctx) says "<fn>: <why>" (fn == nullptr: `why` alone)
static int refuse(kosk_ctx *ctx, const char *fn, const char *why)
{
    ctx->clear_err();
    ctx->err = fn ? std::string(fn) + ": " + why : std::string(why);
    ctx->c->err = ctx->err;
    return -1;
}
// argument validation failed
static int bad_args(const kosk_ctx *, const char *) { return -1; } // read-only entry points leave the error string alone
static int bad_args(kosk_ctx *ctx, const char *fn)
{
    return ctx ? refuse(ctx, fn, "invalid argument (null pointer, batch size out of range, or unsupported for this context)") : -1;
}
// refusals that several entry points share (after bad_args, in this order: armed, stride)
static const char *const WHY_ARMED = "the handle is armed with fewer contexts than this call has proofs (kosk_set_contexts)"; // the call is refused whole
static const char *const WHY_NO_PK_TO_BIND = "not on an armed handle (kosk_set_contexts): instances carry no public key bytes to bind";
static const char *const WHY_SEED_STRIDE = "seed_stride is smaller than one seed (KOSK_SEED_BYTES)";
static const char *const WHY_TAPE_STRIDE = "tape_stride is smaller than one tape (kosk_tape_bytes)";
static const char *const WHY_SALT_STRIDE = "salt_stride is smaller than one salt (32 bytes)";
#define ARMED_CHECK(ctx, n) \
    if ((ctx)->armed && (n) > (ctx)->armed) return refuse(ctx, __func__, WHY_ARMED)

// Batches larger than a sub-context: the chunks (of a sub-context's capacity each) are dealt round-robin to the S
// sub-contexts, which work through theirs concurrently on the handle's lane threads.  With KOSK_STREAMS >= 2 one chunk's
// PCIe transfers (tapes in, 0.68 MB of proof image out per proof; proofs and keys in for the verifier) and host hashing run
// under another chunk's kernels: the streaming write-back of SURVEY.md 8 f4 for a single caller thread.
template <typename F>
static int run_chunks(kosk_ctx *h, int n, F &&fn)
{
    h->clear_err();
    auto on_lane = [&](int i, int first, int count) { return fn(*h->sub[i], first, count); };
    std::vector<std::function<int()>> jobs;
    deal_chunks((int)h->sub.size(), h->sub[0]->own_batch, n, on_lane, jobs); // own_batch: a cohort member's max_batch spans its neighbours' blocks
    return h->run_lanes(jobs);
}
// A call of any n on sub-context 0 alone (the handle's own stream, unmerged), its batch size at a time: fn(c, first, count)
template <typename F>
static int serial_chunks(kosk_ctx *h, int n, F &&fn)
{
    h->clear_err();
    Ctx &c = *h->c;
    for (int first = 0; first < n; first += c.own_batch)
        if (fn(c, first, std::min(n - first, c.own_batch))) return -1;
    return 0;
}

// [p, p + bytes) is page-locked host memory already (kosk_host_alloc, hipHostMalloc, hipHostRegister by the caller): the
// copies can go straight to / from it, no staging and no per-call locking
static bool span_is_pinned(const void *p, size_t bytes)
{
    if (!p || !bytes) return false;
    hipPointerAttribute_t a0{}, a1{};
    if (hipPointerGetAttributes(&a0, p) != hipSuccess ||
        hipPointerGetAttributes(&a1, static_cast<const uint8_t *>(p) + bytes - 1) != hipSuccess) {
        (void)hipGetLastError(); // plain pageable memory: not an error
        return false;
    }
    if (a0.type != hipMemoryTypeHost || a1.type != hipMemoryTypeHost) return false;
    // both ends page-locked is not enough: they must belong to ONE mapping (two registrations with a pageable gap between them,
    // or a neighbour's registration that ends inside the buffer, give unrelated device addresses)
    if (!a0.devicePointer || !a1.devicePointer) return false;
    return static_cast<const uint8_t *>(a1.devicePointer) - static_cast<const uint8_t *>(a0.devicePointer) == (ptrdiff_t)(bytes - 1);
}
// records go straight to / from a buffer the CALLER page-locked (KOSK_REGISTER=0: never), else through the pinned staging buffers
static bool copy_direct(const kosk_ctx *ctx, const void *p, size_t bytes) { return ctx->c->host_register && span_is_pinned(p, bytes); }

// draw n proofs' worth of randomness through the (stateful) callback / OS entropy, sequentially in proof order and in the
// reference's call order and lengths (kosk.cpp:12, mlwe_prover.cpp:9, ss.cpp:5)
static void draw_tapes(const kosk_ctx *ctx, int n, std::vector<uint8_t> &drawn)
{
    const Params &P = ctx->c->P;
    drawn.resize((size_t)n * P.tape_bytes);
    const Ctx &c0 = *ctx->c;
    uint8_t *tp = drawn.data();
    auto draw = [&](size_t len) { if (c0.rb) c0.rb(c0.rb_user, tp, len); else os_randombytes(tp, len); tp += len; };
    for (int b = 0; b < n; b++) {
        draw(64);
        for (int i = 0; i < P.M; i++) draw(32);
        for (int i = 0; i < P.nfresh; i++) draw(302);
    }
}

// Where the randomness of a tape-taking call comes from.  Explicit tapes; seeds (seeded proving: kosk-seedtape-v1, expanded on the
// device); or neither -- then the handle's entropy mode (kosk_set_entropy) decides between the reference's draw sequence for whole
// tapes and one 32-byte draw per proof.  resolve() makes the draws (sequentially, in proof order: the callback is stateful) and
// leaves either `tapes` or `seeds` set.
struct RandSrc {
    const uint8_t *tapes = nullptr;
    size_t tape_stride = 0;
    const uint8_t *seeds = nullptr;
    size_t seed_stride = 0;
    bool seeded = false; // a *_seeded entry point, or tapes == NULL on a handle in KOSK_ENTROPY_SEED mode
    std::vector<uint8_t> drawn;
    RandSrc() = default;
    RandSrc(RandSrc &&) = default;
    ~RandSrc() { host_wipe_vec(drawn); } // drawn tapes / seeds do not go back to the heap readable

    static RandSrc from_tapes(const kosk_ctx *ctx, const uint8_t *tapes, size_t tape_stride)
    {
        RandSrc r;
        r.tapes = tapes;
        r.tape_stride = tape_stride;
        r.seeded = !tapes && ctx->c->entropy_seed;
        return r;
    }
    static RandSrc from_seeds(const uint8_t *seeds, size_t seed_stride)
    {
        RandSrc r;
        r.seeds = seeds;
        r.seed_stride = seed_stride;
        r.seeded = true;
        return r;
    }
    // the tape-taking entry point, or its *_seeded twin
    static RandSrc of(const kosk_ctx *ctx, bool seeded_call, const uint8_t *rand, size_t stride)
    {
        return seeded_call ? from_seeds(rand, stride) : from_tapes(ctx, rand, stride);
    }
    // draw_tapes_too: false leaves a NULL tape pointer alone (the callee draws inside a single sub-context's call)
    void resolve(const kosk_ctx *ctx, int n, bool draw_tapes_too = true)
    {
        if (seeded && !seeds) {
            drawn.resize((size_t)n * SEED_BYTES);
            draw_seeds(*ctx->c, n, drawn.data());
            seeds = drawn.data();
            seed_stride = SEED_BYTES;
        } else if (!seeded && !tapes && draw_tapes_too) {
            draw_tapes(ctx, n, drawn);
            tapes = drawn.data();
            tape_stride = ctx->c->P.tape_bytes;
        }
    }
    // the part of this source that serves proofs [first, ...) of the call
    KeygenIn part(const Params &P, int first, uint8_t *pk, uint8_t *sk) const
    {
        KeygenIn kg{tapes ? tapes + (size_t)first * tape_stride : nullptr, tape_stride, pk + (size_t)first * P.pk_bytes, sk + (size_t)first * P.sk_bytes};
        if (seeded) { kg.seeds = seeds + (size_t)first * seed_stride; kg.seed_stride = seed_stride; }
        return kg;
    }
};
// proofs [first, first + count) of the caller's call on sub-context c: position b of the call uses context b
static int prove_at(Ctx &c, int first, int count, const KeygenIn *kg = nullptr)
{
    c.bind_first = first;
    return prove_resident(c, count, false, kg);
}

static thread_local std::string g_create_err; // error text of the last failed kosk_create on this thread

#define HIPCHK_C(x) KOSK_HIPCHK(x)

extern "C" {

size_t kosk_pk_bytes(int k) { Params p; return make_params(k, p) ? p.pk_bytes : 0; }
size_t kosk_sk_bytes(int k) { Params p; return make_params(k, p) ? p.sk_bytes : 0; }
size_t kosk_proof_bytes(int k) { Params p; return make_params(k, p) ? p.proof_bytes : 0; }
size_t kosk_tape_bytes(int k) { Params p; return make_params(k, p) ? p.tape_bytes : 0; }
int kosk_tape_from_seed(int k, const uint8_t seed[KOSK_SEED_BYTES], uint8_t *tape)
{
    Params p;
    if (!make_params(k, p) || !seed || !tape) return -1;
    tape_from_seed(p, seed, tape);
    return 0;
}
int kosk_proof_field(int k, int idx, size_t *offset, size_t *size)
{
    Params p;
    if (!make_params(k, p) || idx < 0 || idx >= NFIELDS) return -1;
    if (offset) *offset = p.off[idx];
    if (size) *size = p.size[idx];
    return 0;
}

void kosk_options_init(kosk_options *opt)
{
    if (!opt) return;
    memset(opt, 0, sizeof *opt);
    opt->size = (uint32_t)sizeof *opt;
    opt->combine_wait_us = opt->combine_idle_us = opt->combine_prewake_us = -1;
    opt->strict_encoding = opt->fs_mode = opt->blocking_sync = opt->hooks_unmerged = -1;
}
int kosk_create(kosk_ctx **ctx, int device, int kyber_k, int max_batch) { return kosk_create_ex(ctx, device, kyber_k, max_batch, nullptr); }

int kosk_create_ex(kosk_ctx **ctx, int device, int kyber_k, int max_batch, const kosk_options *user_opt)
{
    if (!ctx) return -1;
    *ctx = nullptr;
    kosk_ctx *h = nullptr;
    try {
        g_create_err.clear();
        kosk_options o;
        kosk_options_init(&o);
        if (user_opt) { // a caller compiled against a shorter (older) struct leaves the tail at "not given"
            if (user_opt->size < 8 || user_opt->size > 4096) { g_create_err = "kosk_create_ex: options.size is not set (call kosk_options_init first)"; return -1; }
            memcpy(&o, user_opt, std::min<size_t>(user_opt->size, sizeof o));
            o.size = (uint32_t)sizeof o;
        }
        CtxOpts co_;
        co_.host_threads = o.host_threads > 0 ? o.host_threads : 0;
        co_.blocking_sync = o.blocking_sync;
        co_.strict_encoding = o.strict_encoding;
        co_.fs_device = o.fs_mode < 0 ? -1 : (o.fs_mode == KOSK_FS_DEVICE ? 1 : 0);
        if (const char *e = getenv("AMD_DIRECT_DISPATCH"))
            if (atoi(e) == 0 && e[0] != '\0') {
                // measured on ROCm 7.2 (tools/stress.py): with direct dispatch off, hipStreamSynchronize returned before
                // device-to-host copies into pinned memory had landed; the host then hashed stale digests
                g_create_err = "AMD_DIRECT_DISPATCH=0 is not supported: stream synchronisation does not cover D2H copies in that mode";
                return -1;
            }
        int S = 1; // streams: sub-batches in flight per handle (1 measured best at 46 proofs: kernels sit on latency floors)
        if (o.streams > 0) S = o.streams;
        if (S > max_batch) S = max_batch > 0 ? max_batch : 1;
        if (S > 8) S = 8;
        h = new kosk_ctx();
        h->max_batch = max_batch;
        h->hooks_unmerged = o.hooks_unmerged > 0;
        int W = 1; // combine: handles per cohort (needs streams = 1)
        if (o.combine > 0) W = o.combine > Combiner::MAX_WIDTH ? Combiner::MAX_WIDTH : o.combine;
        if (W > 1 && S == 1 && max_batch >= 1) {
            std::lock_guard<std::mutex> lk(g_cohort_mu);
            Cohort *co = nullptr;
            int idx = -1;
            for (Cohort *x : g_cohorts)
                if (x->device == device && x->k == kyber_k && x->per == max_batch && x->comb->width() == W && x->opts.host_threads == co_.host_threads &&
                    x->opts.blocking_sync == co_.blocking_sync && x->opts.strict_encoding == co_.strict_encoding && x->opts.fs_device == co_.fs_device &&
                    (idx = x->comb->join()) >= 0) { co = x; break; }
            if (!co) {
                std::unique_ptr<Cohort> fresh(new Cohort());
                fresh->device = device; fresh->k = kyber_k; fresh->per = max_batch; fresh->opts = co_;
                int wait_us = 5000, idle_us = 1000;
                if (o.combine_wait_us >= 0) wait_us = o.combine_wait_us;
                if (o.combine_idle_us >= 0) idle_us = o.combine_idle_us;
                int prewake_us = 400; // how long a member whose run has announced its end may spin for it (0: members sleep to the end)
                if (o.combine_prewake_us >= 0) prewake_us = o.combine_prewake_us;
                fresh->comb.reset(new Combiner(W, wait_us, idle_us, prewake_us));
                fresh->member.assign((size_t)W, nullptr);
                if ((long)W * max_batch > 1 << 20) { g_create_err = "combine x max_batch too large"; delete h; return -1; }
                if (ctx_create(&fresh->arena, device, kyber_k, W * max_batch, g_create_err, 1, co_)) { delete h; return -1; }
                if (ensure_verify_workspace(*fresh->arena)) { // views share it: allocated with the arena, not on first use
                    g_create_err = fresh->arena->err;
                    delete fresh->arena;
                    delete h;
                    return -1;
                }
                idx = fresh->comb->join();
                co = fresh.release();
                g_cohorts.push_back(co);
            }
            Ctx *v = nullptr;
            // Host workers: a full run is led by member 0 and hashes W callers' tables, so member 0 gets W callers' worth; the
            // other members only ever lead partial runs (start-up, stragglers) and make do with one caller's worth -- a
            // process with many cohorts (one per rank on an 8-GPU node) stays far below any thread limit
            if (ctx_make_view(*co->arena, idx * max_batch, max_batch, co->arena->base_threads * (idx == 0 ? W : 1), &v, g_create_err)) {
                if (co->comb->leave(idx) == 0) {
                    delete co->arena;
                    g_cohorts.erase(std::remove(g_cohorts.begin(), g_cohorts.end(), co), g_cohorts.end());
                    delete co;
                }
                delete h;
                return -1;
            }
            h->sub.push_back(v);
            h->c = v;
            h->cohort = co;
            h->member_i = idx;
            co->member[idx] = h;
            *ctx = h;
            return 0;
        }
        const int per = (max_batch + S - 1) / S;
        for (int i = 0; i < S; i++) {
            Ctx *c = nullptr;
            if (ctx_create(&c, device, kyber_k, per, g_create_err, S, co_)) {
                delete h;
                return -1;
            }
            h->sub.push_back(c);
        }
        h->c = h->sub[0];
        // the lane threads live as long as the handle: a batch call never creates a thread
        h->lanes.create(S - 1);
        *ctx = h;
        return 0;
    } catch (const std::exception &e) {
        try { g_create_err = std::string("kosk_create: ") + e.what(); } catch (...) {}
    } catch (...) {
        try { g_create_err = "kosk_create: unknown exception"; } catch (...) {}
    }
    try { delete h; } catch (...) {}
    return -1;
}
void kosk_destroy(kosk_ctx *ctx)
{
    if (!ctx) return;
    try { delete ctx; } catch (...) {}
}
const char *kosk_last_error(const kosk_ctx *ctx)
{
    if (!ctx) return g_create_err.c_str();
    return ctx->err.empty() ? ctx->c->err.c_str() : ctx->err.c_str();
}
int kosk_set_randombytes(kosk_ctx *ctx, kosk_randombytes_fn fn, void *user)
{
    if (!ctx) return -1;
    for (Ctx *c : ctx->sub) { c->rb = fn; c->rb_user = user; }
    return 0;
}

int kosk_set_contexts(kosk_ctx *ctx, int n, const uint8_t *contexts, size_t context_stride)
{
    if (!ctx) return -1;
    GUARD(ctx)
    ctx->clear_err();
    if (n == 0) { ctx->disarm(); return 0; }
    if (n < 0 || !contexts) return refuse(ctx, __func__, "n contexts need n >= 1 and a pointer (n = 0 disarms)");
    if (context_stride < 32) return refuse(ctx, __func__, "context_stride is smaller than one context (32 bytes)");
    Ctx &c = *ctx->c;
    HIPCHK_C(hipSetDevice(c.device));
    uint8_t *d = nullptr;
    // allocated and filled before the old state goes: a failure leaves the handle armed as it was
    HIPCHK_C((hipError_t)c.inv.raw_alloc(reinterpret_cast<void **>(&d), (size_t)n * 32, 0));
    const hipError_t e = hipMemcpy2D(d, 32, contexts, context_stride, 32, (size_t)n, is_device_pointer(contexts) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
    if (e != hipSuccess) { c.inv.raw_free(d, 0); HIPCHK_C(e); }
    ctx->disarm();
    c.inv.adopt("d_contexts", &ctx->d_contexts, d, (size_t)n * 32, 0, Inventory::INVG_BIND); // public: the caller's contexts
    ctx->armed = n;
    for (Ctx *x : ctx->sub) { x->bind_ctx = d; x->bind_n = n; x->bind_first = 0; }
    return 0;
    GUARD_END
}

// tests: candidate lists for round 2 of this handle's prover (header).  Refusals leave the lists that were set as they are
int kosk_force_opened_candidates(kosk_ctx *ctx, int n, const uint16_t *cand)
{
    if (!ctx) return -1;
    GUARD(ctx)
    ctx->clear_err();
    if (!cand) { ctx->unforce(); return 0; }
    if (n < 1 || n > KOSK_FORCE_MAX_LISTS) return refuse(ctx, __func__, "n lists need 1 <= n <= KOSK_FORCE_MAX_LISTS (cand == NULL clears)");
    for (size_t i = 0; i < (size_t)n * NOPEN; i++)
        if (cand[i] >= NPARTY) return refuse(ctx, __func__, "a candidate is not a party (every entry must be below 1454)");
    Ctx &c = *ctx->c;
    if (c.use_graphs) return refuse(ctx, __func__, "not on a handle that replays captured graphs (KOSK_GRAPHS=1): their kernel arguments are frozen");
    if (ctx->cohort) return refuse(ctx, __func__, "not on a cohort member (combine): its proofs may run in another member's call");
    HIPCHK_C(hipSetDevice(c.device));
    std::vector<uint16_t> h(cand, cand + (size_t)n * NOPEN);
    uint16_t *d = nullptr;
    HIPCHK_C((hipError_t)c.inv.raw_alloc(reinterpret_cast<void **>(&d), h.size() * sizeof(uint16_t), 0));
    const hipError_t e = hipMemcpy(d, h.data(), h.size() * sizeof(uint16_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) { c.inv.raw_free(d, 0); HIPCHK_C(e); }
    ctx->unforce();
    ctx->h_force.swap(h);
    c.inv.adopt("d_force", &ctx->d_force, d, ctx->h_force.size() * sizeof(uint16_t), 0, Inventory::INVG_FORCE); // public: the test's candidate lists
    for (Ctx *x : ctx->sub) { x->force_d = d; x->force_h = ctx->h_force.data(); x->force_n = n; }
    return 0;
    GUARD_END
}
// the host's function behind the PRF on one list, no handle (tests that run without a GPU)
int kosk_opened_tables(const uint16_t cand[150], uint16_t *sel, uint16_t *rest, int sel_stride)
{
    if (!cand || !sel || !rest || sel_stride < NREST || sel_stride < SEL_OPOS + NOPEN) return -1;
    for (int i = 0; i < NOPEN; i++)
        if (cand[i] >= NPARTY) return -1;
    try {
        opened_from_candidates(cand, sel, rest);
        opened_derived_tables(sel, rest);
    } catch (...) { return -1; }
    return 0;
}

int kosk_set_entropy(kosk_ctx *ctx, int mode)
{
    if (!ctx) return -1;
    if (mode != KOSK_ENTROPY_TAPE && mode != KOSK_ENTROPY_SEED) return bad_args(ctx, __func__);
    for (Ctx *c : ctx->sub) c->entropy_seed = mode == KOSK_ENTROPY_SEED;
    return 0;
}

// The tape-taking entry points and their *_seeded twins differ in one stride check and in the RandSrc they make: one body per pair, with
// the entry point's name for the messages.  `rand`: tapes or seeds
static int stage_prover_inputs_src(kosk_ctx *ctx, const char *fn, int n, bool seeded, const uint8_t *rand, size_t stride, uint8_t *pk, uint8_t *sk)
{
    if (!ctx || n < 1 || n > ctx->max_batch) return bad_args(ctx, fn);
    if (seeded && rand && stride < SEED_BYTES) return refuse(ctx, fn, WHY_SEED_STRIDE);
    return guard(ctx, fn, [&]() -> int {
        const Params &P = ctx->c->P;
        RandSrc src = RandSrc::of(ctx, seeded, rand, stride);
        src.resolve(ctx, n); // the randombytes callback is stateful: draw everything sequentially, then stage in parallel
        return ctx->run(n, [&](Ctx &c, int first, int count) {
            const KeygenIn kg = src.part(P, first, pk, sk);
            return stage_prover_inputs(c, count, kg.tapes, kg.tape_stride, kg.pk, kg.sk, kg.seeds, kg.seed_stride);
        });
    });
}
// The resident fetch / stage calls in wire format `fmt`.  (The image calls have always refused n = 0 and the packed ones taken it as
// nothing to do; the table of every entry point's checks is in DESIGN.md 31)
static int fetch_fmt(kosk_ctx *ctx, const char *fn, int n, int fmt, uint8_t *out)
{
    if (!ctx || n < (fmt == FMT_IMAGE ? 1 : 0) || n > ctx->max_batch || !out) return bad_args(ctx, fn);
    return guard(ctx, fn, [&]() -> int {
        const size_t rb = format_bytes(ctx->c->P, fmt);
        return ctx->run(n, [&](Ctx &c, int first, int count) { return fetch_proofs(c, count, fmt, out + (size_t)first * rb); });
    });
}
static int stage_fmt(kosk_ctx *ctx, const char *fn, int n, int fmt, const uint8_t *in, const uint8_t *pk)
{
    if (!ctx || n < (fmt == FMT_IMAGE ? 1 : 0) || n > ctx->max_batch || !in || !pk) return bad_args(ctx, fn);
    return guard(ctx, fn, [&]() -> int {
        const Params &P = ctx->c->P;
        const size_t rb = format_bytes(P, fmt);
        return ctx->run(n, [&](Ctx &c, int first, int count) {
            return stage_verifier_inputs(c, count, fmt, in + (size_t)first * rb, pk + (size_t)first * P.pk_bytes);
        });
    });
}
int kosk_stage_prover_inputs(kosk_ctx *ctx, int n, const uint8_t *tapes, size_t tape_stride, uint8_t *pk, uint8_t *sk)
{
    return stage_prover_inputs_src(ctx, __func__, n, false, tapes, tape_stride, pk, sk);
}
int kosk_stage_prover_inputs_seeded(kosk_ctx *ctx, int n, const uint8_t *seeds, size_t seed_stride, uint8_t *pk, uint8_t *sk)
{
    return stage_prover_inputs_src(ctx, __func__, n, true, seeds, seed_stride, pk, sk);
}
int kosk_prove_resident(kosk_ctx *ctx, int n)
{
    if (!ctx || n < 1 || n > ctx->max_batch) return bad_args(ctx, __func__);
    ARMED_CHECK(ctx, n);
    WGUARD(ctx)
    return ctx->run(n, [&](Ctx &c, int first, int count) { return prove_at(c, first, count); });
    WGUARD_END
}
int kosk_fetch_proofs(kosk_ctx *ctx, int n, uint8_t *pi) { return fetch_fmt(ctx, __func__, n, FMT_IMAGE, pi); }
int kosk_fetch_proofs_compact(kosk_ctx *ctx, int n, uint8_t *out) { return fetch_fmt(ctx, __func__, n, FMT_COMPACT, out); }
int kosk_fetch_proofs_dense(kosk_ctx *ctx, int n, uint8_t *out) { return fetch_fmt(ctx, __func__, n, FMT_DENSE, out); }
int kosk_stage_verifier_inputs(kosk_ctx *ctx, int n, const uint8_t *pi, const uint8_t *pk) { return stage_fmt(ctx, __func__, n, FMT_IMAGE, pi, pk); }
int kosk_stage_verifier_inputs_compact(kosk_ctx *ctx, int n, const uint8_t *in, const uint8_t *pk) { return stage_fmt(ctx, __func__, n, FMT_COMPACT, in, pk); }
int kosk_stage_verifier_inputs_dense(kosk_ctx *ctx, int n, const uint8_t *in, const uint8_t *pk) { return stage_fmt(ctx, __func__, n, FMT_DENSE, in, pk); }

// verify `count` resident proofs of sub-context c and file their fail masks at the caller's proof index `first`
static int verify_into(kosk_ctx *ctx, Ctx &c, int first, int count, uint8_t *ok, int pk_mode, const uint8_t *pk)
{
    c.bind_first = first; // an armed handle: position b of the call is checked under context b
    if (verify_resident(c, count, ok + first, pk_mode, pk)) return -1;
    memcpy(ctx->masks.data() + first, c.h_fail, sizeof(uint32_t) * (size_t)count);
    return 0;
}
// every verify entry point: the masks of an earlier call are gone, whatever happens next
static void reset_masks(kosk_ctx *ctx, int n)
{
    ctx->masks_n = 0;
    ctx->masks.assign((size_t)n, 0);
    ctx->verify_keys = 0;
}
// a verify call completed: what kosk_kem_enc_verified may rely on
static void note_verified_keys(kosk_ctx *ctx, int kind)
{
    ctx->verify_keys = kind;
    ctx->verify_epoch = ctx->c->pk_epoch;
}

int kosk_verify_resident(kosk_ctx *ctx, int n, uint8_t *ok)
{
    if (!ctx || n < 1 || n > ctx->max_batch || !ok) return bad_args(ctx, __func__);
    ARMED_CHECK(ctx, n);
    GUARD(ctx)
    reset_masks(ctx, n);
    if (ctx->run(n, [&](Ctx &c, int first, int count) { return verify_into(ctx, c, first, count, ok, 0, nullptr); })) return -1;
    ctx->masks_n = n;
    note_verified_keys(ctx, ctx->c->resident_pk_n >= n && ctx->c->keys_from_pk_n >= n ? 1 : 3);
    return 0;
    GUARD_END
}

// ---- merged resident calls of a cohort (KOSK_COMBINE) ----
struct KeygenCall { const uint8_t *tapes; size_t tape_stride; uint8_t *pk, *sk; const uint8_t *seeds; size_t seed_stride; };
struct VerifyCall { const uint8_t *pk; uint8_t *ok; };

// what every member of a finished run takes over from the run's leader
static void run_epilogue(Cohort &co, int first, int count, int rc, const Ctx &lead)
{
    for (int k = 0; k < count; k++) {
        kosk_ctx *m = co.member[first + k];
        // what keeps a member in KOSK_WIPE_CALL out of merged runs is CK_ALONE (combined_keygen / combined_verify); this only keeps its
        // solo runs out of kosk_combine_stats, which an armed member's solo runs are counted in (header: kosk_set_wipe)
        if (!(m->wipe_mode && count == 1)) {
            m->merged_calls++;
            m->merged_members += count;
        }
        if (k) memcpy(m->c->phase_sec, lead.phase_sec, sizeof(lead.phase_sec));
        if (rc) { m->err = lead.err; m->c->err = lead.err; }
    }
}

// Scope of a merged run on its leader's view: while it lives, prove_resident / verify_resident tell the combiner when only their tail
// is left, and the run's other callers wake up for the return instead of sleeping through it (kosk_combine.hpp: near_end).
struct NearEnd {
    Ctx &c;
    NearEnd(Ctx &c_, Cohort &co, int first, int count) : c(c_)
    {
        if (count > 1) {
            Combiner *comb = co.comb.get();
            try { c.near_end_hook = [comb, first] { comb->near_end(first); }; } catch (...) { c.near_end_hook = nullptr; }
        }
    }
    ~NearEnd() { c.near_end_hook = nullptr; }
    NearEnd(const NearEnd &) = delete;
    NearEnd &operator=(const NearEnd &) = delete;
};

// Scope of a run on its leader's view: the view may run `total` proofs (its own block and the blocks of the run's other members
// behind it) with the host workers of `count` callers; both go back to one caller's worth however the run ends.
struct RunScope {
    Ctx &c;
    RunScope(Ctx &c_, int count, int total) : c(c_)
    {
        c.call_cap = std::min(std::max(total, c.own_batch), c.max_batch);
        c.nthreads = std::min(c.base_threads * count, c.reserved_threads); // a call never creates threads
    }
    ~RunScope() { c.call_cap = c.own_batch; c.nthreads = c.base_threads; }
    RunScope(const RunScope &) = delete;
    RunScope &operator=(const RunScope &) = delete;
};

static int combined_keygen(kosk_ctx *h, int n, const KeygenCall &call)
{
    Cohort &co = *h->cohort;
    h->clear_err();
    // a caller's bad arguments fail THAT caller, here, not the run it would have joined (and every innocent member of it)
    if (call.tapes && call.tape_stride < h->c->P.tape_bytes) return refuse(h, nullptr, "tape_stride is smaller than one proof's tape (kosk_tape_bytes)");
    CombineReq r;
    // the stateful randombytes callback is per handle: a call that draws whole tapes through it runs alone (a seeded call's seeds were
    // drawn by its own caller before it got here, and the entropy source is not part of what makes calls mergeable)
    r.kind = (call.tapes || call.seeds) ? CK_KEYGEN : CK_ALONE;
    if (h->hooks_unmerged && h->c->round_hook) r.kind = CK_ALONE; // the hook must fire on this caller's own thread (kosk_options::hooks_unmerged)
    if (h->armed) r.kind = CK_ALONE; // bound proofs (kosk_set_contexts) stay out of merged runs: binding is not part of what makes calls mergeable
    if (h->wipe_mode) r.kind = CK_ALONE; // KOSK_WIPE_CALL: the member wipes its own block when its call ends, so the call is its own run
    h->c->bind_first = 0;
    r.n = n;
    r.full = n == co.per;
    r.args = const_cast<KeygenCall *>(&call);
    std::string what;
    const int rc = co.comb->call(h->member_i, r, [&co](int first, int count, const CombineReq *const *reqs) -> int {
        Ctx &c = *co.member[first]->c; // the run leader's view: this thread is its caller
        std::vector<KeygenIn> segs((size_t)count);
        int total = 0;
        for (int k = 0; k < count; k++) {
            const KeygenCall *a = static_cast<const KeygenCall *>(reqs[k]->args);
            const Ctx &mv = *co.member[first + k]->c; // round hooks are per handle: every member's fires with its own block of the tables
            segs[k] = KeygenIn{a->tapes, a->tape_stride, a->pk, a->sk, reqs[k]->n, k + 1 < count ? &segs[k + 1] : nullptr, mv.round_hook, mv.round_user,
                               a->seeds, a->seed_stride};
            total += reqs[k]->n;
        }
        NearEnd ne(c, co, first, count);
        int rc;
        {
            RunScope scope(c, count, total);
            rc = prove_resident(c, total, false, &segs[0]);
        }
        for (int k = 0; k < count; k++) {
            Ctx &v = *co.member[first + k]->c;
            v.resident_pk_n = rc ? 0 : reqs[k]->n;
            // a merged run either copied every member's tapes into its own block of the tape buffer or read the callers' device
            // buffers in place: either way a later kosk_prove_resident on this member must not assume anything
            if (count > 1) v.tape_cur = nullptr;
        }
        run_epilogue(co, first, count, rc, c);
        return rc;
    }, &what);
    if (rc == -2) { h->err = "exception in a merged call: " + what; h->c->err = h->err; return -1; }
    return rc;
}

static int combined_verify(kosk_ctx *h, int n, const VerifyCall &call)
{
    Cohort &co = *h->cohort;
    h->clear_err();
    h->masks_n = 0;
    if (!call.pk && h->c->resident_pk_n < n)
        return refuse(h, nullptr, "no resident public keys for this batch: pk == NULL needs a key generation (or a verifier staging call) of at least n proofs on this context");
    CombineReq r;
    r.kind = call.pk ? CK_VERIFY_PK_GIVEN : CK_VERIFY_PK_RESIDENT;
    if (h->hooks_unmerged && h->c->round_hook) r.kind = CK_ALONE;
    if (h->armed || h->wipe_mode) r.kind = CK_ALONE; // as in combined_keygen
    h->c->bind_first = 0;
    r.n = n;
    r.full = n == co.per;
    r.args = const_cast<VerifyCall *>(&call);
    std::string what;
    const int rc = co.comb->call(h->member_i, r, [&co](int first, int count, const CombineReq *const *reqs) -> int {
        Ctx &c = *co.member[first]->c;
        std::vector<VerifySeg> segs((size_t)count);
        int total = 0;
        bool given = false;
        for (int k = 0; k < count; k++) {
            const VerifyCall *a = static_cast<const VerifyCall *>(reqs[k]->args);
            const Ctx &mv = *co.member[first + k]->c;
            segs[k] = VerifySeg{reqs[k]->n, a->pk, a->ok, k + 1 < count ? &segs[k + 1] : nullptr, mv.round_hook, mv.round_user};
            total += reqs[k]->n;
            given = a->pk != nullptr;
        }
        const int keep = c.resident_pk_n;
        if (!given) c.resident_pk_n = total; // every member checked its own keys before it posted
        NearEnd ne(c, co, first, count);
        int rc;
        {
            struct KeepPk { Ctx &c; int keep; bool on; ~KeepPk() { if (on) c.resident_pk_n = keep; } } keep_pk{c, keep, !given};
            RunScope scope(c, count, total);
            rc = verify_resident(c, total, nullptr, given ? 1 : 2, nullptr, &segs[0]);
        }
        int off = 0;
        for (int k = 0; k < count; k++) {
            kosk_ctx *m = co.member[first + k];
            m->masks.assign((size_t)reqs[k]->n, 0);
            if (!rc) {
                memcpy(m->masks.data(), c.h_fail + off, sizeof(uint32_t) * (size_t)reqs[k]->n);
                m->masks_n = reqs[k]->n;
                if (given) m->c->resident_pk_n = reqs[k]->n;
            }
            off += reqs[k]->n;
        }
        run_epilogue(co, first, count, rc, c);
        return rc;
    }, &what);
    if (rc == -2) { h->err = "exception in a merged call: " + what; h->c->err = h->err; return -1; }
    return rc;
}

static int keygen_resident_src(kosk_ctx *ctx, const char *fn, int n, bool seeded, const uint8_t *rand, size_t stride, uint8_t *pk, uint8_t *sk)
{
    if (!ctx || n < 1 || n > ctx->max_batch || !pk || !sk) return bad_args(ctx, fn);
    if (ctx->armed && n > ctx->armed) return refuse(ctx, fn, WHY_ARMED);
    if (seeded && rand && stride < SEED_BYTES) return refuse(ctx, fn, WHY_SEED_STRIDE);
    return guard(ctx, fn, [&]() -> int { return wiped_call(ctx, [&]() -> int {
        RandSrc src = RandSrc::of(ctx, seeded, rand, stride);
        // stateful callback: seeds are drawn here, on the caller's own thread and in proof order, whatever serves the call afterwards; whole
        // tapes only where the sub-batches of the call run in parallel (one sub-context draws its own inside its call)
        src.resolve(ctx, n, !ctx->cohort && ctx->sub.size() > 1);
        if (ctx->cohort) return combined_keygen(ctx, n, KeygenCall{src.tapes, src.tape_stride, pk, sk, src.seeds, src.seed_stride});
        const Params &P = ctx->c->P;
        return ctx->run(n, [&](Ctx &c, int first, int count) {
            const KeygenIn kg = src.part(P, first, pk, sk);
            return prove_at(c, first, count, &kg);
        });
    }); });
}
int kosk_verifiable_keygen_resident(kosk_ctx *ctx, int n, const uint8_t *tapes, size_t tape_stride, uint8_t *pk, uint8_t *sk)
{
    return keygen_resident_src(ctx, __func__, n, false, tapes, tape_stride, pk, sk);
}
int kosk_verifiable_keygen_seeded_resident(kosk_ctx *ctx, int n, const uint8_t *seeds, size_t seed_stride, uint8_t *pk, uint8_t *sk)
{
    return keygen_resident_src(ctx, __func__, n, true, seeds, seed_stride, pk, sk);
}
int kosk_tape_expand_device(kosk_ctx *ctx, int n, const uint8_t *seeds, size_t seed_stride, uint8_t *d_tapes, size_t tape_stride)
{
    if (!ctx || n < 1 || n > ctx->max_batch || !seeds || !d_tapes) return bad_args(ctx, __func__);
    if (seed_stride < SEED_BYTES) return refuse(ctx, __func__, WHY_SEED_STRIDE);
    WGUARD(ctx)
    ctx->clear_err();
    return tape_expand_device(*ctx->c, n, seeds, seed_stride, d_tapes, tape_stride);
    WGUARD_END
}
int kosk_verify_resident_pk(kosk_ctx *ctx, int n, const uint8_t *pk, uint8_t *ok)
{
    if (!ctx || n < 1 || n > ctx->max_batch || !ok) return bad_args(ctx, __func__);
    ARMED_CHECK(ctx, n);
    GUARD(ctx)
    if (ctx->cohort) return combined_verify(ctx, n, VerifyCall{pk, ok});
    const Params &P = ctx->c->P;
    reset_masks(ctx, n);
    if (ctx->run(n, [&](Ctx &c, int first, int count) {
            return verify_into(ctx, c, first, count, ok, pk ? 1 : 2, pk ? pk + (size_t)first * P.pk_bytes : nullptr);
        })) return -1;
    ctx->masks_n = n;
    note_verified_keys(ctx, 1);
    return 0;
    GUARD_END
}
int kosk_set_round_hook(kosk_ctx *ctx, kosk_round_fn fn, void *user)
{
    if (!ctx) return -1;
    GUARD(ctx)
    if (fn && ctx->sub.size() > 1) return refuse(ctx, nullptr, "kosk_set_round_hook needs streams = 1 (one digest table per round)");
    for (Ctx *c : ctx->sub) { c->round_hook = fn; c->round_user = user; }
    return 0;
    GUARD_END
}
int kosk_resident_digests(kosk_ctx *ctx, int round, void **d_digests, size_t *stride)
{
    if (!ctx || round < 0 || round > 1) return bad_args(ctx, __func__);
    GUARD(ctx)
    if (ctx->sub.size() > 1) return refuse(ctx, nullptr, "kosk_resident_digests needs streams = 1 (sub-batches keep separate tables)");
    if (d_digests) *d_digests = round ? ctx->c->d_dig2 : ctx->c->d_dig1;
    if (stride) *stride = (size_t)NPARTY * 32;
    return 0;
    GUARD_END
}

// ---- the host-buffer calls, proofs in wire format `fmt` ----
// image: the raw struct image.  compact: packed / unpacked on the GPU, so PCIe carries 78 % of the image bytes in each
// direction.  dense, kosk-dense-v1 (kosk_dense.hip): packed by the same kernel on the dense field plan; unpacked and
// refilled (rows 407..1303 of the seven low-degree fields) on the GPU behind the H2D copy.  Same chunking and lanes for all three
static int keygen_batch_from(kosk_ctx *ctx, int n, RandSrc &src, uint8_t *pk, uint8_t *sk, uint8_t *out, int fmt)
{
    const Params &P = ctx->c->P;
    const size_t rb = format_bytes(P, fmt);
    src.resolve(ctx, n); // stateful callback: everything sequentially, in proof order, then the chunks in parallel
    const bool direct = copy_direct(ctx, out, (size_t)n * rb);
    return run_chunks(ctx, n, [&](Ctx &c, int first, int count) {
        const KeygenIn kg = src.part(P, first, pk, sk);
        if (prove_at(c, first, count, &kg)) return -1;
        return fetch_proofs(c, count, fmt, out + (size_t)first * rb, direct);
    });
}
static int keygen_batch_src(kosk_ctx *ctx, const char *fn, int n, bool seeded, const uint8_t *rand, size_t stride, uint8_t *pk, uint8_t *sk, uint8_t *out, int fmt)
{
    if (!ctx || n < 0 || !pk || !sk || !out) return bad_args(ctx, fn);
    if (ctx->armed && n > ctx->armed) return refuse(ctx, fn, WHY_ARMED);
    if (seeded && rand && stride < SEED_BYTES) return refuse(ctx, fn, WHY_SEED_STRIDE);
    if (n == 0) return 0;
    return guard(ctx, fn, [&]() -> int { return wiped_call(ctx, [&]() -> int {
        RandSrc src = RandSrc::of(ctx, seeded, rand, stride);
        return keygen_batch_from(ctx, n, src, pk, sk, out, fmt);
    }); });
}
static int verify_batch_fmt(kosk_ctx *ctx, const char *fn, int n, int fmt, const uint8_t *in, const uint8_t *pk, uint8_t *ok)
{
    if (!ctx || n < 0 || !in || !pk || !ok) return bad_args(ctx, fn);
    if (ctx->armed && n > ctx->armed) return refuse(ctx, fn, WHY_ARMED);
    if (n == 0) { ctx->masks_n = 0; return 0; }
    return guard(ctx, fn, [&]() -> int {
        const Params &P = ctx->c->P;
        const size_t rb = format_bytes(P, fmt);
        reset_masks(ctx, n);
        const bool direct = copy_direct(ctx, in, (size_t)n * rb);
        const int rc = run_chunks(ctx, n, [&](Ctx &c, int first, int count) {
            const uint8_t *src = in + (size_t)first * rb;
            c.host_img = nullptr;
            if (stage_verifier_inputs(c, count, fmt, src, pk + (size_t)first * P.pk_bytes, direct)) return -1;
            if (fmt == FMT_IMAGE) {
                // the verifier's host reads the unopened parties' digests straight from the caller's images: nothing to copy back for them
                // (verify_resident takes the pointer and clears it first thing)
                c.host_img = src;
                c.host_img_stride = P.proof_bytes;
            }
            return verify_into(ctx, c, first, count, ok, 0, nullptr);
        });
        if (!rc) { ctx->masks_n = n; note_verified_keys(ctx, n > ctx->c->own_batch ? 2 : 1); }
        return rc;
    });
}
int kosk_verifiable_keygen_batch(kosk_ctx *ctx, int n, const uint8_t *tapes, size_t tape_stride, uint8_t *pk, uint8_t *sk, uint8_t *pi)
{
    return keygen_batch_src(ctx, __func__, n, false, tapes, tape_stride, pk, sk, pi, FMT_IMAGE);
}
int kosk_verifiable_keygen_seeded_batch(kosk_ctx *ctx, int n, const uint8_t *seeds, size_t seed_stride, uint8_t *pk, uint8_t *sk, uint8_t *pi)
{
    return keygen_batch_src(ctx, __func__, n, true, seeds, seed_stride, pk, sk, pi, FMT_IMAGE);
}
int kosk_verifiable_keygen_batch_compact(kosk_ctx *ctx, int n, const uint8_t *tapes, size_t tape_stride, uint8_t *pk, uint8_t *sk, uint8_t *out)
{
    return keygen_batch_src(ctx, __func__, n, false, tapes, tape_stride, pk, sk, out, FMT_COMPACT);
}
int kosk_verifiable_keygen_seeded_batch_compact(kosk_ctx *ctx, int n, const uint8_t *seeds, size_t seed_stride, uint8_t *pk, uint8_t *sk, uint8_t *out)
{
    return keygen_batch_src(ctx, __func__, n, true, seeds, seed_stride, pk, sk, out, FMT_COMPACT);
}
int kosk_verifiable_keygen_batch_dense(kosk_ctx *ctx, int n, const uint8_t *tapes, size_t tape_stride, uint8_t *pk, uint8_t *sk, uint8_t *out)
{
    return keygen_batch_src(ctx, __func__, n, false, tapes, tape_stride, pk, sk, out, FMT_DENSE);
}
int kosk_verifiable_keygen_seeded_batch_dense(kosk_ctx *ctx, int n, const uint8_t *seeds, size_t seed_stride, uint8_t *pk, uint8_t *sk, uint8_t *out)
{
    return keygen_batch_src(ctx, __func__, n, true, seeds, seed_stride, pk, sk, out, FMT_DENSE);
}
int kosk_verify_batch(kosk_ctx *ctx, int n, const uint8_t *pi, const uint8_t *pk, uint8_t *ok) { return verify_batch_fmt(ctx, __func__, n, FMT_IMAGE, pi, pk, ok); }
int kosk_verify_batch_compact(kosk_ctx *ctx, int n, const uint8_t *in, const uint8_t *pk, uint8_t *ok) { return verify_batch_fmt(ctx, __func__, n, FMT_COMPACT, in, pk, ok); }
int kosk_verify_batch_dense(kosk_ctx *ctx, int n, const uint8_t *in, const uint8_t *pk, uint8_t *ok) { return verify_batch_fmt(ctx, __func__, n, FMT_DENSE, in, pk, ok); }

// ---- the same five calls with the packed format as an argument (KOSK_FMT_COMPACT, KOSK_FMT_DENSE, KOSK_FMT_DENSE2): the bodies above, so
// a further format needs no further names.  Anything else, the image included (it has the unsuffixed calls), is refused
static const char WHY_FMT[] = "unknown format: a _fmt call takes KOSK_FMT_COMPACT, KOSK_FMT_DENSE or KOSK_FMT_DENSE2";
static bool packed_fmt(int fmt) { return fmt == FMT_COMPACT || fmt == FMT_DENSE || fmt == FMT_DENSE2; }
int kosk_verifiable_keygen_batch_fmt(kosk_ctx *ctx, int fmt, int n, const uint8_t *tapes, size_t tape_stride, uint8_t *pk, uint8_t *sk, uint8_t *out)
{
    if (!ctx) return -1;
    if (!packed_fmt(fmt)) return refuse(ctx, __func__, WHY_FMT);
    return keygen_batch_src(ctx, __func__, n, false, tapes, tape_stride, pk, sk, out, fmt);
}
int kosk_verifiable_keygen_seeded_batch_fmt(kosk_ctx *ctx, int fmt, int n, const uint8_t *seeds, size_t seed_stride, uint8_t *pk, uint8_t *sk, uint8_t *out)
{
    if (!ctx) return -1;
    if (!packed_fmt(fmt)) return refuse(ctx, __func__, WHY_FMT);
    return keygen_batch_src(ctx, __func__, n, true, seeds, seed_stride, pk, sk, out, fmt);
}
int kosk_verify_batch_fmt(kosk_ctx *ctx, int fmt, int n, const uint8_t *in, const uint8_t *pk, uint8_t *ok)
{
    if (!ctx) return -1;
    if (!packed_fmt(fmt)) return refuse(ctx, __func__, WHY_FMT);
    return verify_batch_fmt(ctx, __func__, n, fmt, in, pk, ok);
}
int kosk_fetch_proofs_fmt(kosk_ctx *ctx, int fmt, int n, uint8_t *out)
{
    if (!ctx) return -1;
    if (!packed_fmt(fmt)) return refuse(ctx, __func__, WHY_FMT);
    return fetch_fmt(ctx, __func__, n, fmt, out);
}
int kosk_stage_verifier_inputs_fmt(kosk_ctx *ctx, int fmt, int n, const uint8_t *in, const uint8_t *pk)
{
    if (!ctx) return -1;
    if (!packed_fmt(fmt)) return refuse(ctx, __func__, WHY_FMT);
    return stage_fmt(ctx, __func__, n, fmt, in, pk);
}

// ---- second-level entry points (kosk_split.cpp) -----------------------------------------------------------
size_t kosk_randomness_bytes(int k) { Params p; return make_params(k, p) ? randomness_bytes(p) : 0; }
size_t kosk_range_proof_bytes(int k) { Params p; return make_params(k, p) ? range_proof_bytes(p) : 0; }
size_t kosk_mlwe_inst_bytes(int k) { Params p; return make_params(k, p) ? mlwe_inst_bytes(p) : 0; }

int kosk_prepare_randomness(kosk_ctx *ctx, int n, const uint8_t *tapes, size_t tape_stride, uint8_t *rand_out)
{
    if (!ctx || n < 0 || !rand_out) return bad_args(ctx, __func__);
    WGUARD(ctx)
    return serial_chunks(ctx, n, [&](Ctx &c, int first, int count) {
        return prepare_randomness(c, count, tapes ? tapes + (size_t)first * tape_stride : nullptr, tape_stride, rand_out + (size_t)first * randomness_bytes(c.P));
    });
    WGUARD_END
}
int kosk_prepare_range_proof(kosk_ctx *ctx, int n, const uint8_t *tapes, size_t tape_stride, uint8_t *range_out)
{
    if (!ctx || n < 0 || !range_out) return bad_args(ctx, __func__);
    WGUARD(ctx)
    return serial_chunks(ctx, n, [&](Ctx &c, int first, int count) {
        return prepare_range_proof(c, count, tapes ? tapes + (size_t)first * tape_stride : nullptr, tape_stride, range_out + (size_t)first * range_proof_bytes(c.P));
    });
    WGUARD_END
}
int kosk_prove_prepared(kosk_ctx *ctx, int n, const uint8_t *inst, const uint8_t *rand_in, const uint8_t *range_in,
                        const uint8_t *tapes, size_t tape_stride, uint8_t *pi)
{
    if (!ctx || n < 0 || !inst || !rand_in || !range_in || !pi) return bad_args(ctx, __func__);
    if (ctx->armed) return refuse(ctx, __func__, WHY_NO_PK_TO_BIND);
    WGUARD(ctx)
    return serial_chunks(ctx, n, [&](Ctx &c, int first, int count) {
        c.bind_first = first; // (forced candidate lists are indexed by the position in the call)
        return prove_prepared(c, count, inst + (size_t)first * mlwe_inst_bytes(c.P), rand_in + (size_t)first * randomness_bytes(c.P),
                              range_in + (size_t)first * range_proof_bytes(c.P), tapes ? tapes + (size_t)first * tape_stride : nullptr,
                              tape_stride, pi + (size_t)first * c.P.proof_bytes);
    });
    WGUARD_END
}
int kosk_verify_inst(kosk_ctx *ctx, int n, const uint8_t *pi, const uint8_t *inst, uint8_t *ok)
{
    if (!ctx || n < 0 || !pi || !inst || !ok) return bad_args(ctx, __func__);
    if (ctx->armed) return refuse(ctx, __func__, WHY_NO_PK_TO_BIND);
    GUARD(ctx)
    reset_masks(ctx, n);
    if (serial_chunks(ctx, n, [&](Ctx &c, int first, int count) {
            if (stage_verifier_inst(c, count, pi + (size_t)first * c.P.proof_bytes, inst + (size_t)first * mlwe_inst_bytes(c.P))) return -1;
            return verify_into(ctx, c, first, count, ok, 0, nullptr);
        })) return -1;
    ctx->masks_n = n;
    note_verified_keys(ctx, 3);
    return 0;
    GUARD_END
}

// ---- compact wire format (kosk_compact.hip) ------------------------------------------------------------------
size_t kosk_compact_proof_bytes(int k) { Params p; return make_params(k, p) ? make_compact_plan(p).bytes : 0; }
int kosk_proof_compress(int k, const uint8_t *pi, uint8_t *out)
{
    Params p;
    if (!make_params(k, p) || !pi || !out) return -1;
    return guard(static_cast<const kosk_ctx *>(nullptr), __func__, [&]() -> int {
    return compact_encode(p, pi, out);
    GUARD_END
}
int kosk_proof_decompress(int k, const uint8_t *in, uint8_t *pi)
{
    Params p;
    if (!make_params(k, p) || !pi || !in) return -1;
    return guard(static_cast<const kosk_ctx *>(nullptr), __func__, [&]() -> int {
    compact_decode(p, in, pi);
    return 0;
    GUARD_END
}

// ---- dense wire format kosk-dense-v1 (kosk_dense.hip) --------------------------------------------------------------
size_t kosk_dense_proof_bytes(int k) { Params p; return make_params(k, p) ? make_dense_plan(p).bytes : 0; }
int kosk_proof_dense_pack(int k, const uint8_t *pi, uint8_t *out)
{
    Params p;
    if (!make_params(k, p) || !pi || !out) return -1;
    return guard(static_cast<const kosk_ctx *>(nullptr), __func__, [&]() -> int {
    return dense_encode(p, pi, out);
    GUARD_END
}
int kosk_proof_dense_unpack(int k, const uint8_t *in, uint8_t *pi)
{
    Params p;
    if (!make_params(k, p) || !pi || !in) return -1;
    return guard(static_cast<const kosk_ctx *>(nullptr), __func__, [&]() -> int {
    return dense_decode(p, in, pi);
    GUARD_END
}
int kosk_dense_fill_device(kosk_ctx *ctx, int n, uint8_t *d_images, size_t image_stride, uint32_t *d_status)
{
    if (!ctx || n < 1 || !d_images || !d_status) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    return dense_fill_device(*ctx->c, n, d_images, image_stride, d_status);
    GUARD_END
}
int kosk_dense_check_device(kosk_ctx *ctx, int n, const uint8_t *d_images, size_t image_stride, uint32_t *d_status)
{
    if (!ctx || n < 1 || !d_images || !d_status) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    return dense_fill_device(*ctx->c, n, const_cast<uint8_t *>(d_images), image_stride, d_status, true); // the check kernel takes them const
    GUARD_END
}

// ---- dense wire format kosk-dense-v2 (kosk_dense.hip): the same codec and kernels on the second field plan ----
size_t kosk_dense2_proof_bytes(int k) { Params p; return make_params(k, p) ? make_dense_plan(p, FMT_DENSE2).bytes : 0; }
int kosk_proof_dense2_pack(int k, const uint8_t *pi, uint8_t *out)
{
    Params p;
    if (!make_params(k, p) || !pi || !out) return -1;
    return guard(static_cast<const kosk_ctx *>(nullptr), __func__, [&]() -> int {
    return dense_encode(p, pi, out, FMT_DENSE2);
    GUARD_END
}
int kosk_proof_dense2_unpack(int k, const uint8_t *in, uint8_t *pi)
{
    Params p;
    if (!make_params(k, p) || !pi || !in) return -1;
    return guard(static_cast<const kosk_ctx *>(nullptr), __func__, [&]() -> int {
    return dense_decode(p, in, pi, FMT_DENSE2);
    GUARD_END
}
int kosk_dense2_fill_device(kosk_ctx *ctx, int n, uint8_t *d_images, size_t image_stride, uint32_t *d_status)
{
    if (!ctx || n < 1 || !d_images || !d_status) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    return dense_fill_device(*ctx->c, n, d_images, image_stride, d_status, false, FMT_DENSE2);
    GUARD_END
}
int kosk_dense2_check_device(kosk_ctx *ctx, int n, const uint8_t *d_images, size_t image_stride, uint32_t *d_status)
{
    if (!ctx || n < 1 || !d_images || !d_status) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    return dense_fill_device(*ctx->c, n, const_cast<uint8_t *>(d_images), image_stride, d_status, true, FMT_DENSE2); // the check kernel takes them const
    GUARD_END
}

// ---- transcoding between the wire formats (kosk_compact.hip: transcode) -----------------------------------------------------------
static_assert((int)KOSK_FMT_IMAGE == (int)FMT_IMAGE && (int)KOSK_FMT_COMPACT == (int)FMT_COMPACT && (int)KOSK_FMT_DENSE == (int)FMT_DENSE && (int)KOSK_FMT_DENSE2 == (int)FMT_DENSE2, "kosk_mi355x.h and kosk_ctx.hpp");
size_t kosk_format_bytes(int k, int fmt) { Params p; return make_params(k, p) ? format_bytes(p, fmt) : 0; }
// unmerged, on sub-context 0 (the handle's own stream), chunks of its batch size; brings no secret onto the handle (no wipe under KOSK_WIPE_CALL)
int kosk_transcode_batch(kosk_ctx *ctx, int n, int from, const uint8_t *in, int to, uint8_t *out, int32_t *status)
{
    if (!ctx) return -1;
    if (!in || !out || !status) return refuse(ctx, __func__, "null pointer");
    if (n < 1) return refuse(ctx, __func__, "n must be at least 1");
    const size_t ib = format_bytes(ctx->c->P, from), ob = format_bytes(ctx->c->P, to);
    if (!ib || !ob) return refuse(ctx, __func__, "unknown format (KOSK_FMT_IMAGE, KOSK_FMT_COMPACT, KOSK_FMT_DENSE, KOSK_FMT_DENSE2)");
    if (from == to) return refuse(ctx, __func__, "from and to are the same format");
    const uintptr_t i0 = reinterpret_cast<uintptr_t>(in), o0 = reinterpret_cast<uintptr_t>(out);
    if (i0 < o0 + (size_t)n * ob && o0 < i0 + (size_t)n * ib) return refuse(ctx, __func__, "in and out overlap");
    GUARD(ctx)
    return serial_chunks(ctx, n, [&](Ctx &c, int first, int count) {
        return transcode(c, count, from, in + (size_t)first * ib, to, out + (size_t)first * ob, status + first);
    });
    GUARD_END
}

int kosk_verify_fail_masks(const kosk_ctx *ctx, uint32_t *masks, int n)
{
    // only the masks of the LAST verify call, and only if it completed: never stale entries of an earlier, larger batch
    if (!ctx || !masks || n < 0 || n > ctx->masks_n) return bad_args(ctx, __func__);
    memcpy(masks, ctx->masks.data(), sizeof(uint32_t) * (size_t)n);
    return 0;
}

// ---- Kyber KEM (kosk_kem_kernels.hip) ------------------------------------------------------------------------
size_t kosk_ct_bytes(int k) { return k == 2 ? 768 : k == 3 ? 1088 : k == 4 ? 1568 : 0; }

// the m of crypto_kem_enc_derand for n items: the caller's, or one 32-byte draw per item, in item order, on the caller's thread
// (kem.c:117-118)
static const uint8_t *kem_coins(const kosk_ctx *ctx, int n, const uint8_t *coins, std::vector<uint8_t> &drawn)
{
    if (coins) return coins;
    drawn.resize((size_t)n * 32);
    draw_seeds(*ctx->c, n, drawn.data());
    return drawn.data();
}
// a KEM call of any n as launch groups of at most KEM_CHUNK items, unmerged, on sub-context 0 (the handle's own stream)
static int kem_chunks(kosk_ctx *ctx, int n, const std::function<int(Ctx &, int, int)> &fn)
{
    ctx->clear_err();
    Ctx &c = *ctx->c;
    for (int first = 0; first < n; first += KEM_CHUNK) {
        const int count = n - first < KEM_CHUNK ? n - first : KEM_CHUNK;
        if (fn(c, first, count)) { ctx->err = c.err; return -1; }
    }
    return 0;
}
int kosk_kem_enc_batch(kosk_ctx *ctx, int n, const uint8_t *pk, const uint8_t *coins, uint8_t *ct, uint8_t *ss)
{
    if (!ctx || n < 1 || !pk || !ct || !ss) return bad_args(ctx, __func__);
    WGUARD(ctx)
    const Params &P = ctx->c->P;
    const size_t ctb = kosk_ct_bytes(P.K);
    std::vector<uint8_t> drawn;
    VecWiper<uint8_t> drawn_gone(drawn);
    const uint8_t *m = kem_coins(ctx, n, coins, drawn);
    return kem_chunks(ctx, n, [&](Ctx &c, int first, int count) {
        return kem_enc(c, count, pk + (size_t)first * P.pk_bytes, m + (size_t)first * 32, ct + (size_t)first * ctb, ss + (size_t)first * 32);
    });
    WGUARD_END
}
int kosk_kem_dec_batch(kosk_ctx *ctx, int n, const uint8_t *ct, const uint8_t *sk, uint8_t *ss)
{
    if (!ctx || n < 1 || !ct || !sk || !ss) return bad_args(ctx, __func__);
    WGUARD(ctx)
    const Params &P = ctx->c->P;
    const size_t ctb = kosk_ct_bytes(P.K);
    return kem_chunks(ctx, n, [&](Ctx &c, int first, int count) {
        return kem_dec(c, count, ct + (size_t)first * ctb, sk + (size_t)first * P.sk_bytes, ss + (size_t)first * 32);
    });
    WGUARD_END
}
// crypto_kem_keypair[_derand] (kem.c:25-57): the caller's coins, or one 64-byte draw (d || z) per item, in item order, on the caller's
// thread (kem.c:53-54).  Only the KEM workspace is written: pk_epoch, the resident keys and verify_keys stay as they are.
int kosk_kem_keypair_batch(kosk_ctx *ctx, int n, const uint8_t *coins, uint8_t *pk, uint8_t *sk)
{
    if (!ctx || n < 1 || !pk || !sk) return bad_args(ctx, __func__);
    WGUARD(ctx)
    const Params &P = ctx->c->P;
    std::vector<uint8_t> drawn;
    VecWiper<uint8_t> drawn_gone(drawn);
    if (!coins) {
        drawn.resize((size_t)n * 64);
        const Ctx &c0 = *ctx->c;
        for (int b = 0; b < n; b++) {
            uint8_t *dst = drawn.data() + (size_t)b * 64;
            if (c0.rb) c0.rb(c0.rb_user, dst, 64);
            else os_randombytes(dst, 64);
        }
        coins = drawn.data();
    }
    return kem_chunks(ctx, n, [&](Ctx &c, int first, int count) {
        return kem_keypair(c, count, coins + (size_t)first * 64, pk + (size_t)first * P.pk_bytes, sk + (size_t)first * P.sk_bytes);
    });
    WGUARD_END
}
static_assert(KOSK_KEYCHK_HASH == KEYCHK_HASH && KOSK_KEYCHK_PK_RANGE == KEYCHK_PK_RANGE && KOSK_KEYCHK_S_RANGE == KEYCHK_S_RANGE, "kosk_mi355x.h and kosk_ctx.hpp");
int kosk_kem_check_pk(kosk_ctx *ctx, int n, const uint8_t *pk, uint8_t *flags)
{
    if (!ctx || n < 1 || !pk || !flags) return bad_args(ctx, __func__);
    GUARD(ctx)
    const Params &P = ctx->c->P;
    return kem_chunks(ctx, n, [&](Ctx &c, int first, int count) { return kem_check(c, count, pk + (size_t)first * P.pk_bytes, 0, flags + first); });
    GUARD_END
}
int kosk_kem_check_sk(kosk_ctx *ctx, int n, const uint8_t *sk, uint8_t *flags)
{
    if (!ctx || n < 1 || !sk || !flags) return bad_args(ctx, __func__);
    WGUARD(ctx)
    const Params &P = ctx->c->P;
    return kem_chunks(ctx, n, [&](Ctx &c, int first, int count) { return kem_check(c, count, sk + (size_t)first * P.sk_bytes, 1, flags + first); });
    WGUARD_END
}
// why the keys of the last verify call cannot serve a call on its first n keys (kosk_kem_enc_verified, kosk_registry_admit_verified); nullptr: they can
static const char *verified_keys_refusal(const kosk_ctx *ctx, int n)
{
    if (ctx->cohort) return "not available with call combining (the handle is a member of a cohort)";
    if (ctx->sub.size() > 1) return "needs streams = 1 (sub-batches keep separate public keys)";
    if (ctx->verify_keys == 0 || ctx->masks_n < 1) return "no verify call has completed on this handle";
    if (ctx->verify_keys == 2) return "the last verify call was a chunked kosk_verify_batch call (n > max_batch): its public keys are not resident as one batch";
    if (ctx->masks_n < n) return "the last verify call covered fewer than n proofs";
    if (ctx->verify_keys == 3) return "the last verify call left no public key bytes in HBM (its A and t came from instances)";
    if (ctx->verify_epoch != ctx->c->pk_epoch || ctx->c->resident_pk_n < n) return "the resident public keys were replaced after the last verify call";
    return nullptr;
}
int kosk_kem_enc_verified(kosk_ctx *ctx, int n, const uint8_t *coins, uint8_t *ct, uint8_t *ss, uint8_t *done)
{
    if (!ctx || n < 1 || !ct || !ss || !done) return bad_args(ctx, __func__);
    WGUARD(ctx)
    ctx->clear_err();
    auto refuse = [&](const char *why) { ctx->err = std::string("kosk_kem_enc_verified: ") + why; ctx->c->err = ctx->err; return -1; };
    if (const char *why = verified_keys_refusal(ctx, n)) return refuse(why);
    // coins are drawn for every position, accepted or not: the draw order does not depend on the outcome
    std::vector<uint8_t> drawn, bits((size_t)n);
    VecWiper<uint8_t> drawn_gone(drawn);
    const uint8_t *m = kem_coins(ctx, n, coins, drawn);
    for (int b = 0; b < n; b++) bits[(size_t)b] = ctx->masks[(size_t)b] == 0;
    const size_t ctb = kosk_ct_bytes(ctx->c->P.K);
    if (kem_chunks(ctx, n, [&](Ctx &c, int first, int count) {
            return kem_enc(c, count, nullptr, m + (size_t)first * 32, ct + (size_t)first * ctb, ss + (size_t)first * 32, bits.data() + first, first);
        })) return -1;
    if (hipMemcpy(done, bits.data(), (size_t)n, hipMemcpyDefault) != hipSuccess) { (void)hipGetLastError(); return refuse("copying the verify bits to `done` failed"); }
    return 0;
    WGUARD_END
}

// ---- KEM with one resident key (kosk_kem_kernels.hip) ----
static_assert((int)KOSK_KEM_KEY_NONE == (int)KEM_KEY_NONE && (int)KOSK_KEM_KEY_PK == (int)KEM_KEY_PK && (int)KOSK_KEM_KEY_SK == (int)KEM_KEY_SK, "kosk_mi355x.h and kosk_ctx.hpp");
int kosk_kem_key_set(kosk_ctx *ctx, const uint8_t *pk, const uint8_t *sk)
{
    if (!ctx || (pk == nullptr) == (sk == nullptr)) return bad_args(ctx, __func__);
    GUARD(ctx) // under KOSK_WIPE_CALL too: the slot this call makes is what it is for
    ctx->clear_err();
    if (kem_key_set(*ctx->c, pk, sk)) { ctx->err = ctx->c->err; return -1; }
    return 0;
    GUARD_END
}
int kosk_kem_key_state(const kosk_ctx *ctx) { return ctx ? kem_key_state(*ctx->c) : -1; }
int kosk_kem_key_clear(kosk_ctx *ctx)
{
    if (!ctx) return -1;
    GUARD(ctx)
    ctx->clear_err();
    if (kem_key_clear(*ctx->c)) { ctx->err = ctx->c->err; return -1; }
    return 0;
    GUARD_END
}
int kosk_kem_enc_key(kosk_ctx *ctx, int n, const uint8_t *coins, uint8_t *ct, uint8_t *ss)
{
    if (!ctx || n < 1 || !ct || !ss) return bad_args(ctx, __func__);
    WGUARD(ctx)
    ctx->clear_err();
    if (kem_key_state(*ctx->c) == KEM_KEY_NONE) { // before any coin is drawn
        ctx->err = "kosk_kem_enc_key: no key is loaded (kosk_kem_key_set)";
        ctx->c->err = ctx->err;
        return -1;
    }
    const size_t ctb = kosk_ct_bytes(ctx->c->P.K);
    std::vector<uint8_t> drawn;
    VecWiper<uint8_t> drawn_gone(drawn);
    const uint8_t *m = kem_coins(ctx, n, coins, drawn);
    return kem_chunks(ctx, n, [&](Ctx &c, int first, int count) {
        return kem_enc_key(c, count, m + (size_t)first * 32, ct + (size_t)first * ctb, ss + (size_t)first * 32);
    });
    WGUARD_END
}
int kosk_kem_dec_key(kosk_ctx *ctx, int n, const uint8_t *ct, uint8_t *ss)
{
    if (!ctx || n < 1 || !ct || !ss) return bad_args(ctx, __func__);
    WGUARD(ctx)
    const size_t ctb = kosk_ct_bytes(ctx->c->P.K);
    return kem_chunks(ctx, n, [&](Ctx &c, int first, int count) {
        return kem_dec_key(c, count, ct + (size_t)first * ctb, ss + (size_t)first * 32);
    });
    WGUARD_END
}

// ---- the verified-key registry (kosk_registry.hip) ----
size_t kosk_registry_slot_bytes(int k) { return k >= 2 && k <= 4 ? registry_slot_bytes(k) : 0; }

// why a call that names `slots` is refused before anything starts; nullptr: the handle has a registry and every value is one of its slots
// (distinct: and none is named twice -- the admissions, where the later writer would be undefined)
static const char *const WHY_HISTORY_FULL = "history is full (kosk_registry_history_reserve): nothing was changed";
static const char *registry_slots_refusal(const kosk_ctx *ctx, int n, const int32_t *slots, bool distinct)
{
    const KemRegistry *r = ctx->c->registry;
    if (!r) return "no registry is reserved (kosk_registry_reserve)";
    for (int b = 0; b < n; b++)
        if (slots[b] < 0 || slots[b] >= r->capacity) return "a slot id outside [0, capacity)";
    if (distinct) {
        std::vector<uint8_t> seen((size_t)r->capacity, 0);
        for (int b = 0; b < n; b++) {
            if (seen[(size_t)slots[b]]) return "a slot id is named twice in one admission";
            seen[(size_t)slots[b]] = 1;
        }
    }
    return nullptr;
}

int kosk_registry_reserve(kosk_ctx *ctx, int capacity)
{
    if (!ctx) return -1;
    GUARD(ctx)
    ctx->clear_err();
    if (registry_reserve(*ctx->c, capacity)) { ctx->err = ctx->c->err; return -1; }
    return 0;
    GUARD_END
}

int kosk_registry_level(const kosk_ctx *ctx, int *used, int *capacity)
{
    if (!ctx) return -1;
    const KemRegistry *r = ctx->c->registry;
    if (used) *used = r ? r->used : 0;
    if (capacity) *capacity = r ? r->capacity : 0;
    return 0;
}

// key b of the call (pk records, or pk == nullptr: the resident keys) into slots[b] where accept[b] != 0 (nullptr: everywhere), in launch groups;
// the mirror follows what the launches wrote.  A launch group that fails (gen_matrix at its block limit) leaves the slots this call wrote empty
// With a history: refused up front where the call's events do not fit; each launch group appends the EVICT events of
// the occupied slots it is about to overwrite in front of its launch (they read the old fingerprints), and the ADMIT events of every
// accepted position follow once every group has succeeded.  The clean-up eviction of a failed call appends nothing: its slots were empty
// before the call, or their EVICT events are in place
static int registry_admit_run(kosk_ctx *ctx, const char *fn, int n, const uint8_t *pk, const uint8_t *accept, const int32_t *slots)
{
    std::vector<int32_t> dst((size_t)n);
    for (int b = 0; b < n; b++) dst[(size_t)b] = !accept || accept[b] ? slots[b] : -1;
    const size_t pkb = ctx->c->P.pk_bytes;
    KemRegistry &r = *ctx->c->registry;
    const bool hist = r.hist_max != 0;
    if (hist) {
        long need = 0;
        for (int b = 0; b < n; b++)
            if (dst[(size_t)b] >= 0) need += r.occ[(size_t)dst[(size_t)b]] ? 2 : 1;
        if (need > (long)r.hist_max - r.hist_size) return refuse(ctx, fn, WHY_HISTORY_FULL);
    }
    std::vector<int32_t> ev_op, ev_slot;
    int done = 0; // keys of completed or started launch groups
    const int rc = kem_chunks(ctx, n, [&](Ctx &c, int first, int count) {
        if (hist) {
            ev_op.clear(); ev_slot.clear();
            for (int b = first; b < first + count; b++)
                if (dst[(size_t)b] >= 0 && r.occ[(size_t)dst[(size_t)b]]) { ev_op.push_back(reghist::OP_EVICT); ev_slot.push_back(dst[(size_t)b]); }
            if (!ev_op.empty() && reghist_append(c, (int)ev_op.size(), ev_op.data(), ev_slot.data())) return -1;
        }
        done = first + count;
        return kem_registry_admit(c, count, pk ? pk + (size_t)first * pkb : nullptr, first, dst.data() + first);
    });
    if (hist && !rc) {
        ev_op.clear(); ev_slot.clear();
        for (int b = 0; b < n; b++)
            if (dst[(size_t)b] >= 0) { ev_op.push_back(reghist::OP_ADMIT); ev_slot.push_back(dst[(size_t)b]); }
        if (!ev_op.empty() && reghist_append(*ctx->c, (int)ev_op.size(), ev_op.data(), ev_slot.data())) { ctx->err = ctx->c->err; return -1; }
    }
    for (int b = 0; b < done; b++) {
        if (dst[(size_t)b] < 0 || r.occ[(size_t)dst[(size_t)b]]) continue; // masked, or a replacement: `used` does not change
        r.occ[(size_t)dst[(size_t)b]] = 1;
        r.used++;
    }
    if (!rc) return 0;
    const std::string why = ctx->err;
    std::vector<int32_t> named;
    for (int b = 0; b < done; b++)
        if (dst[(size_t)b] >= 0) named.push_back(dst[(size_t)b]);
    (void)hipGetLastError();
    (void)registry_evict(*ctx->c, (int)named.size(), named.data());
    ctx->err = why;
    ctx->c->err = why;
    return -1;
}

int kosk_registry_admit_verified(kosk_ctx *ctx, int n, const int32_t *slots, uint8_t *done)
{
    if (!ctx || n < 1 || !slots || !done) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    if (const char *why = registry_slots_refusal(ctx, n, slots, true)) return refuse(ctx, "kosk_registry_admit_verified", why);
    if (const char *why = verified_keys_refusal(ctx, n)) return refuse(ctx, "kosk_registry_admit_verified", why);
    std::vector<uint8_t> bits((size_t)n);
    for (int b = 0; b < n; b++) bits[(size_t)b] = ctx->masks[(size_t)b] == 0;
    if (registry_admit_run(ctx, "kosk_registry_admit_verified", n, nullptr, bits.data(), slots)) return -1;
    memcpy(done, bits.data(), (size_t)n);
    return 0;
    GUARD_END
}

int kosk_registry_admit(kosk_ctx *ctx, int n, const uint8_t *pk, const uint8_t *accept, const int32_t *slots)
{
    if (!ctx || n < 1 || !pk || !slots) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    if (const char *why = registry_slots_refusal(ctx, n, slots, true)) return refuse(ctx, "kosk_registry_admit", why);
    return registry_admit_run(ctx, "kosk_registry_admit", n, pk, accept, slots);
    GUARD_END
}

int kosk_registry_evict(kosk_ctx *ctx, int n, const int32_t *slots)
{
    if (!ctx || n < 1 || !slots) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    if (const char *why = registry_slots_refusal(ctx, n, slots, false)) return refuse(ctx, "kosk_registry_evict", why);
    KemRegistry &r = *ctx->c->registry;
    if (r.hist_max) { // one EVICT per occupied slot at its first occurrence, in front of the wipe: the events read the fingerprints
        std::vector<int32_t> ev_op, ev_slot;
        std::vector<uint8_t> seen((size_t)r.capacity, 0);
        for (int b = 0; b < n; b++) {
            const size_t s = (size_t)slots[b];
            if (!r.occ[s] || seen[s]) continue;
            seen[s] = 1;
            ev_op.push_back(reghist::OP_EVICT); ev_slot.push_back(slots[b]);
        }
        if ((long)ev_op.size() > (long)r.hist_max - r.hist_size) return refuse(ctx, "kosk_registry_evict", WHY_HISTORY_FULL);
        if (!ev_op.empty() && reghist_append(*ctx->c, (int)ev_op.size(), ev_op.data(), ev_slot.data())) { ctx->err = ctx->c->err; return -1; }
    }
    if (registry_evict(*ctx->c, n, slots)) { ctx->err = ctx->c->err; return -1; }
    return 0;
    GUARD_END
}

int kosk_registry_read(kosk_ctx *ctx, int n, const int32_t *slots, uint8_t *state, uint8_t *pk, uint8_t *h)
{
    if (!ctx || n < 1 || !slots || !state) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    if (const char *why = registry_slots_refusal(ctx, n, slots, false)) return refuse(ctx, "kosk_registry_read", why);
    if (registry_read(*ctx->c, n, slots, state, pk, h)) { ctx->err = ctx->c->err; return -1; }
    return 0;
    GUARD_END
}

int kosk_kem_enc_slots(kosk_ctx *ctx, int n, const int32_t *slots, const uint8_t *coins, uint8_t *ct, uint8_t *ss, uint8_t *done)
{
    if (!ctx || n < 1 || !slots || !ct || !ss || !done) return bad_args(ctx, __func__);
    WGUARD(ctx)
    ctx->clear_err();
    if (const char *why = registry_slots_refusal(ctx, n, slots, false)) return refuse(ctx, "kosk_kem_enc_slots", why); // before any coin is drawn
    // coins are drawn for every position, occupied or not: the draw order does not depend on the registry
    std::vector<uint8_t> drawn, bits((size_t)n);
    VecWiper<uint8_t> drawn_gone(drawn);
    const uint8_t *m = kem_coins(ctx, n, coins, drawn);
    const KemRegistry &r = *ctx->c->registry;
    for (int b = 0; b < n; b++) bits[(size_t)b] = r.occ[(size_t)slots[b]];
    const size_t ctb = kosk_ct_bytes(ctx->c->P.K);
    if (kem_chunks(ctx, n, [&](Ctx &c, int first, int count) {
            return kem_enc_slots(c, count, slots + first, m + (size_t)first * 32, ct + (size_t)first * ctb, ss + (size_t)first * 32);
        })) return -1;
    if (hipMemcpy(done, bits.data(), (size_t)n, hipMemcpyDefault) != hipSuccess) { (void)hipGetLastError(); return refuse(ctx, "kosk_kem_enc_slots", "copying the occupancy bits to `done` failed"); }
    return 0;
    WGUARD_END
}

// ---- the registry by fingerprint (kosk_registry.hip) ----
static_assert((int)KOSK_ENROL_REJECTED == (int)ENROL_REJECTED && (int)KOSK_ENROL_ADMITTED == (int)ENROL_ADMITTED && (int)KOSK_ENROL_DUPLICATE == (int)ENROL_DUPLICATE,
              "kosk_mi355x.h and kosk_registry_resolve.hpp");
static const char *const WHY_NO_REGISTRY = "no registry is reserved (kosk_registry_reserve)";
size_t kosk_registry_index_entries(int capacity) { return registry_index_entries(capacity); }
int kosk_registry_index_home(int capacity, const uint8_t *h) { return capacity < 1 || !h ? -1 : (int)registry_index_home(capacity, h); }

int kosk_registry_find(kosk_ctx *ctx, int n, const uint8_t *h, int32_t *slots)
{
    if (!ctx || n < 1 || !h || !slots) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    if (!ctx->c->registry) return refuse(ctx, "kosk_registry_find", WHY_NO_REGISTRY);
    return kem_chunks(ctx, n, [&](Ctx &c, int first, int count) { return kem_registry_find(c, count, h + (size_t)first * 32, slots + first); });
    GUARD_END
}

// candidates b of the call (pk records, or pk == nullptr: the resident keys) where accept[b] != 0: fingerprints and hits to the host, the
// resolver, then the admission of the ADMITTED positions through registry_admit_run
static int registry_enrol_run(kosk_ctx *ctx, const char *fn, int n, const uint8_t *pk, const uint8_t *accept, int32_t *slots, uint8_t *status)
{
    const size_t pkb = ctx->c->P.pk_bytes;
    std::vector<uint8_t> fp((size_t)n * 32), all;
    std::vector<int32_t> hit((size_t)n);
    if (kem_chunks(ctx, n, [&](Ctx &c, int first, int count) {
            return kem_registry_probe(c, count, pk ? pk + (size_t)first * pkb : nullptr, first, fp.data() + (size_t)first * 32, hit.data() + first);
        })) return -1;
    if (!accept) { all.assign((size_t)n, 1); accept = all.data(); }
    std::vector<int32_t> dst;
    std::vector<uint8_t> st;
    const int admitted = registry_enrol_resolve(n, accept, fp.data(), hit.data(), ctx->c->registry->occ, dst, st);
    if (admitted < 0) return refuse(ctx, fn, "registry is full (more new keys than empty slots): nothing was changed");
    if (admitted) {
        std::vector<uint8_t> take((size_t)n);
        std::vector<int32_t> named(dst); // a position that is not admitted names no slot: registry_admit_run masks it
        for (int b = 0; b < n; b++) take[(size_t)b] = st[(size_t)b] == ENROL_ADMITTED;
        if (registry_admit_run(ctx, fn, n, pk, take.data(), named.data())) return -1;
    }
    memcpy(slots, dst.data(), sizeof(int32_t) * (size_t)n);
    memcpy(status, st.data(), (size_t)n);
    return 0;
}

int kosk_registry_enrol_verified(kosk_ctx *ctx, int n, int32_t *slots, uint8_t *status)
{
    if (!ctx || n < 1 || !slots || !status) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    if (!ctx->c->registry) return refuse(ctx, "kosk_registry_enrol_verified", WHY_NO_REGISTRY);
    if (const char *why = verified_keys_refusal(ctx, n)) return refuse(ctx, "kosk_registry_enrol_verified", why);
    std::vector<uint8_t> bits((size_t)n);
    for (int b = 0; b < n; b++) bits[(size_t)b] = ctx->masks[(size_t)b] == 0;
    return registry_enrol_run(ctx, "kosk_registry_enrol_verified", n, nullptr, bits.data(), slots, status);
    GUARD_END
}

int kosk_registry_enrol(kosk_ctx *ctx, int n, const uint8_t *pk, const uint8_t *accept, int32_t *slots, uint8_t *status)
{
    if (!ctx || n < 1 || !pk || !slots || !status) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    if (!ctx->c->registry) return refuse(ctx, "kosk_registry_enrol", WHY_NO_REGISTRY);
    return registry_enrol_run(ctx, "kosk_registry_enrol", n, pk, accept, slots, status);
    GUARD_END
}

int kosk_kem_enc_peers(kosk_ctx *ctx, int n, const uint8_t *h, const uint8_t *coins, uint8_t *ct, uint8_t *ss, uint8_t *done)
{
    if (!ctx || n < 1 || !h || !ct || !ss || !done) return bad_args(ctx, __func__);
    WGUARD(ctx)
    ctx->clear_err();
    if (!ctx->c->registry) return refuse(ctx, "kosk_kem_enc_peers", WHY_NO_REGISTRY); // before any coin is drawn
    // coins are drawn for every position, found or not: the draw order does not depend on the registry
    std::vector<uint8_t> drawn;
    VecWiper<uint8_t> drawn_gone(drawn);
    const uint8_t *m = kem_coins(ctx, n, coins, drawn);
    const size_t ctb = kosk_ct_bytes(ctx->c->P.K);
    return kem_chunks(ctx, n, [&](Ctx &c, int first, int count) {
        return kem_enc_peers(c, count, h + (size_t)first * 32, m + (size_t)first * 32, ct + (size_t)first * ctb, ss + (size_t)first * 32, done + first);
    });
    WGUARD_END
}

// ---- the registry tree, format kosk-regtree-v1 (kosk_regtree.hpp, kosk_registry.hip) ----
static_assert((int)KOSK_REGTREE_TIER_LEVELS == (int)regtree::TIER_LEVELS, "kosk_mi355x.h and kosk_regtree.hpp");
int kosk_registry_tree_depth(int capacity) { return regtree::depth(capacity); }
size_t kosk_registry_tree_bytes(int capacity) { return regtree::tree_bytes(capacity); }
int kosk_regtree_leaf(int kyber_k, const uint8_t *h, uint8_t out[32]) { return regtree::leaf(kyber_k, h, out); }
int kosk_regtree_node(const uint8_t l[32], const uint8_t r[32], uint8_t out[32]) { return regtree::node(l, r, out); }
int kosk_regtree_root_from_path(int kyber_k, int depth, int32_t slot, const uint8_t *h, const uint8_t *path, uint8_t root[32])
{
    return regtree::root_from_path(kyber_k, depth, slot, h, path, root);
}

int kosk_registry_root(kosk_ctx *ctx, uint8_t root[32], int *used, int *capacity)
{
    if (!ctx || !root) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    if (!ctx->c->registry) return refuse(ctx, "kosk_registry_root", WHY_NO_REGISTRY);
    if (registry_root(*ctx->c, root)) { ctx->err = ctx->c->err; return -1; }
    if (used) *used = ctx->c->registry->used;
    if (capacity) *capacity = ctx->c->registry->capacity;
    return 0;
    GUARD_END
}

int kosk_registry_prove_slots(kosk_ctx *ctx, int n, const int32_t *slots, uint8_t *state, uint8_t *h, uint8_t *paths, uint8_t *root)
{
    if (!ctx || n < 1 || !slots || !state) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    if (const char *why = registry_slots_refusal(ctx, n, slots, false)) return refuse(ctx, "kosk_registry_prove_slots", why);
    const KemRegistry &r = *ctx->c->registry;
    const size_t rec = (size_t)regtree::depth(r.capacity) * 32;
    if (rec && !paths) return bad_args(ctx, __func__);
    if (kem_chunks(ctx, n, [&](Ctx &c, int first, int count) {
            return kem_registry_prove(c, count, slots + first, nullptr, h ? h + (size_t)first * 32 : nullptr, nullptr, nullptr, paths ? paths + (size_t)first * rec : nullptr);
        })) return -1;
    for (int b = 0; b < n; b++) state[b] = r.occ[(size_t)slots[b]];
    if (root && registry_root(*ctx->c, root)) { ctx->err = ctx->c->err; return -1; }
    return 0;
    GUARD_END
}

int kosk_registry_prove_peers(kosk_ctx *ctx, int n, const uint8_t *h, int32_t *slots, uint8_t *paths, uint8_t *done, uint8_t *root)
{
    if (!ctx || n < 1 || !h || !slots || !done) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    if (!ctx->c->registry) return refuse(ctx, "kosk_registry_prove_peers", WHY_NO_REGISTRY);
    const size_t rec = (size_t)regtree::depth(ctx->c->registry->capacity) * 32;
    if (rec && !paths) return bad_args(ctx, __func__);
    if (kem_chunks(ctx, n, [&](Ctx &c, int first, int count) {
            return kem_registry_prove(c, count, nullptr, h + (size_t)first * 32, nullptr, slots + first, done + first, paths ? paths + (size_t)first * rec : nullptr);
        })) return -1;
    if (root && registry_root(*ctx->c, root)) { ctx->err = ctx->c->err; return -1; }
    return 0;
    GUARD_END
}

// ---- the sorted tree, format kosk-regsort-v1 (kosk_regsort.hpp, kosk_regsort.hip) ----
size_t kosk_regsort_proof_bytes(int depth) { return regsort::proof_bytes(depth); }
int kosk_regsort_leaf(int kyber_k, const uint8_t *h, int32_t slot, uint8_t out[32]) { return regsort::leaf(kyber_k, h, slot, out); }
int kosk_regsort_node(const uint8_t l[32], const uint8_t r[32], uint8_t out[32]) { return regsort::node(l, r, out); }
int kosk_regsort_root_from_path(int kyber_k, int depth, int32_t pos, const uint8_t *h, int32_t slot, const uint8_t *path, uint8_t root[32])
{
    return regsort::root_from_path(kyber_k, depth, pos, h, slot, path, root);
}
int kosk_regsort_check_proof(int kyber_k, int depth, const uint8_t x[32], const uint8_t *record, const uint8_t root[32])
{
    return regsort::check_proof(kyber_k, depth, x, record, root);
}

int kosk_registry_sorted_root(kosk_ctx *ctx, uint8_t root[32], int *used, int *capacity)
{
    if (!ctx || !root) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    if (!ctx->c->registry) return refuse(ctx, "kosk_registry_sorted_root", WHY_NO_REGISTRY);
    if (registry_sorted_root(*ctx->c, root)) { ctx->err = ctx->c->err; return -1; }
    if (used) *used = ctx->c->registry->used;
    if (capacity) *capacity = ctx->c->registry->capacity;
    return 0;
    GUARD_END
}

int kosk_registry_prove_absent(kosk_ctx *ctx, int n, const uint8_t *h, uint8_t *kind, uint8_t *records, uint8_t *root)
{
    if (!ctx || n < 1 || !h || !kind || !records) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    if (!ctx->c->registry) return refuse(ctx, "kosk_registry_prove_absent", WHY_NO_REGISTRY);
    const size_t rec = regsort::proof_bytes(regtree::depth(ctx->c->registry->capacity));
    if (kem_chunks(ctx, n, [&](Ctx &c, int first, int count) {
            return registry_prove_absent(c, count, h + (size_t)first * 32, kind + first, records + (size_t)first * rec);
        })) return -1;
    if (root && registry_sorted_root(*ctx->c, root)) { ctx->err = ctx->c->err; return -1; }
    return 0;
    GUARD_END
}

int kosk_regsort_order_device(kosk_ctx *ctx, int n, const uint8_t *d_h, const uint8_t *d_flag, int32_t *d_order)
{
    if (!ctx || n < 1 || n > (1 << 24) || !d_h || !d_flag || !d_order || ((uintptr_t)d_h & 7) || ((uintptr_t)d_order & 3)) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    if (regsort_order_device(*ctx->c, n, d_h, d_flag, d_order)) { ctx->err = ctx->c->err; return -1; }
    return 0;
    GUARD_END
}

// ---- the registry history, format kosk-reghist-v1 (kosk_reghist.hpp, kosk_reghist.hip) ----
static_assert((int)KOSK_REGHIST_TIER_LEVELS == (int)reghist::TIER_LEVELS && (int)KOSK_REGHIST_EVENT_BYTES == (int)reghist::EVENT_BYTES &&
              (int)KOSK_REGHIST_ADMIT == (int)reghist::OP_ADMIT && (int)KOSK_REGHIST_EVICT == (int)reghist::OP_EVICT &&
              (int)KOSK_REGHIST_CHECKPOINT == (int)reghist::OP_CHECKPOINT, "kosk_mi355x.h and kosk_reghist.hpp");
static const char *const WHY_NO_HISTORY = "no history is reserved (kosk_registry_history_reserve)";
int kosk_reghist_depth(int size) { return reghist::depth(size); }
size_t kosk_reghist_path_bytes(int size) { return reghist::path_bytes(size); }
size_t kosk_reghist_consistency_bytes(int size) { return reghist::consistency_bytes(size); }
int kosk_reghist_leaf(int kyber_k, const uint8_t event[80], uint8_t out[32]) { return reghist::leaf(kyber_k, event, out); }
int kosk_reghist_node(const uint8_t l[32], const uint8_t r[32], uint8_t out[32]) { return reghist::node(l, r, out); }
int kosk_reghist_empty_root(int kyber_k, uint8_t out[32]) { return reghist::empty_root(kyber_k, out); }
int kosk_reghist_root_from_path(int index, int size, const uint8_t leaf[32], const uint8_t *record, uint8_t root[32])
{
    return reghist::root_from_path(index, size, leaf, record, root);
}
int kosk_reghist_check_consistency(int old_size, int size, const uint8_t root_old[32], const uint8_t root_new[32], const uint8_t *record)
{
    return reghist::check_consistency(old_size, size, root_old, root_new, record);
}

int kosk_registry_history_reserve(kosk_ctx *ctx, int max_events)
{
    if (!ctx) return -1;
    GUARD(ctx)
    ctx->clear_err();
    const KemRegistry *r = ctx->c->registry;
    if (!r) return refuse(ctx, "kosk_registry_history_reserve", WHY_NO_REGISTRY);
    if (max_events < 0 || max_events > reghist::MAX_EVENTS) return refuse(ctx, "kosk_registry_history_reserve", "max_events outside 0 .. 2^24");
    if (max_events && r->hist_size) return refuse(ctx, "kosk_registry_history_reserve", "the history has events: only 0 (free) is allowed");
    if (max_events && r->used) return refuse(ctx, "kosk_registry_history_reserve", "the registry is not empty (kosk_registry_evict): replay from event 0 would be incomplete");
    if (reghist_reserve(*ctx->c, max_events)) { ctx->err = ctx->c->err; return -1; }
    return 0;
    GUARD_END
}

int kosk_registry_history_level(const kosk_ctx *ctx, int *size, int *max_events)
{
    if (!ctx) return -1;
    const KemRegistry *r = ctx->c->registry;
    if (size) *size = r ? r->hist_size : 0;
    if (max_events) *max_events = r ? r->hist_max : 0;
    return 0;
}

// why a history call is refused before anything starts; nullptr: there is a history and `size` (resolved: < 0 is the current size) is one of its sizes
static const char *history_refusal(const kosk_ctx *ctx, int &size)
{
    const KemRegistry *r = ctx->c->registry;
    if (!r) return WHY_NO_REGISTRY;
    if (!r->hist_max) return WHY_NO_HISTORY;
    if (size < 0) size = r->hist_size;
    if (size > r->hist_size) return "size is above the current size of the history";
    return nullptr;
}

int kosk_registry_history_head(kosk_ctx *ctx, int size, uint8_t root[32], int *size_out)
{
    if (!ctx || !root) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    if (const char *why = history_refusal(ctx, size)) return refuse(ctx, "kosk_registry_history_head", why);
    if (reghist_head(*ctx->c, size, root)) { ctx->err = ctx->c->err; return -1; }
    if (size_out) *size_out = size;
    return 0;
    GUARD_END
}

int kosk_registry_history_checkpoint(kosk_ctx *ctx, int *index)
{
    if (!ctx) return -1;
    GUARD(ctx)
    ctx->clear_err();
    int size = -1;
    if (const char *why = history_refusal(ctx, size)) return refuse(ctx, "kosk_registry_history_checkpoint", why);
    if (size >= ctx->c->registry->hist_max) return refuse(ctx, "kosk_registry_history_checkpoint", WHY_HISTORY_FULL);
    if (reghist_checkpoint(*ctx->c, index)) { ctx->err = ctx->c->err; return -1; }
    return 0;
    GUARD_END
}

int kosk_registry_history_read(kosk_ctx *ctx, int first, int n, uint8_t *events)
{
    if (!ctx || n < 1 || first < 0 || !events) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    int size = -1;
    if (const char *why = history_refusal(ctx, size)) return refuse(ctx, "kosk_registry_history_read", why);
    if ((long)first + n > size) return refuse(ctx, "kosk_registry_history_read", "events outside [0, size)");
    if (reghist_read(*ctx->c, first, n, events)) { ctx->err = ctx->c->err; return -1; }
    return 0;
    GUARD_END
}

int kosk_registry_history_prove_events(kosk_ctx *ctx, int size, int n, const int32_t *index, uint8_t *leaves, uint8_t *records, uint8_t *root)
{
    if (!ctx || n < 1 || !index || !records) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    if (const char *why = history_refusal(ctx, size)) return refuse(ctx, "kosk_registry_history_prove_events", why);
    for (int b = 0; b < n; b++)
        if (index[b] < 0 || index[b] >= size) return refuse(ctx, "kosk_registry_history_prove_events", "an index outside [0, size)");
    const size_t rec = reghist::path_bytes(size);
    if (kem_chunks(ctx, n, [&](Ctx &c, int first, int count) {
            return reghist_prove(c, 0, size, count, index + first, leaves ? leaves + (size_t)first * 32 : nullptr, records + (size_t)first * rec);
        })) return -1;
    if (root && reghist_head(*ctx->c, size, root)) { ctx->err = ctx->c->err; return -1; }
    return 0;
    GUARD_END
}

int kosk_registry_history_prove_consistency(kosk_ctx *ctx, int size, int n, const int32_t *old_size, uint8_t *records, uint8_t *root)
{
    if (!ctx || n < 1 || !old_size) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    if (const char *why = history_refusal(ctx, size)) return refuse(ctx, "kosk_registry_history_prove_consistency", why);
    for (int b = 0; b < n; b++)
        if (old_size[b] < 0 || old_size[b] > size) return refuse(ctx, "kosk_registry_history_prove_consistency", "an old size outside [0, size]");
    const size_t rec = reghist::consistency_bytes(size); // 0 for the empty history: no record is written
    if (rec && !records) return bad_args(ctx, __func__);
    if (rec && kem_chunks(ctx, n, [&](Ctx &c, int first, int count) {
            return reghist_prove(c, 1, size, count, old_size + first, nullptr, records + (size_t)first * rec);
        })) return -1;
    if (root && reghist_head(*ctx->c, size, root)) { ctx->err = ctx->c->err; return -1; }
    return 0;
    GUARD_END
}

// ---- the registry monitor (kosk_monitor.hip) ----
static_assert((int)KOSK_MONITOR_OK == (int)MONITOR_OK && (int)KOSK_MONITOR_BAD_RECORD == (int)MONITOR_BAD_RECORD && (int)KOSK_MONITOR_BAD_SLOT == (int)MONITOR_BAD_SLOT &&
              (int)KOSK_MONITOR_ADMIT_OCCUPIED == (int)MONITOR_ADMIT_OCCUPIED && (int)KOSK_MONITOR_EVICT_EMPTY == (int)MONITOR_EVICT_EMPTY &&
              (int)KOSK_MONITOR_EVICT_MISMATCH == (int)MONITOR_EVICT_MISMATCH && (int)KOSK_MONITOR_CP_USED == (int)MONITOR_CP_USED &&
              (int)KOSK_MONITOR_CP_CAPACITY == (int)MONITOR_CP_CAPACITY && (int)KOSK_MONITOR_CP_SLOT_ROOT == (int)MONITOR_CP_SLOT_ROOT &&
              (int)KOSK_MONITOR_CP_SORTED_ROOT == (int)MONITOR_CP_SORTED_ROOT, "kosk_mi355x.h and kosk_ctx.hpp");
static const char *const WHY_NO_MONITOR = "no monitor is reserved (kosk_monitor_reserve)";

int kosk_monitor_reserve(kosk_ctx *ctx, int capacity, int max_events)
{
    if (!ctx) return -1;
    GUARD(ctx)
    ctx->clear_err();
    if (capacity < 0) return refuse(ctx, "kosk_monitor_reserve", "capacity < 0");
    if (max_events < 0 || max_events > reghist::MAX_EVENTS) return refuse(ctx, "kosk_monitor_reserve", "max_events outside 0 .. 2^24");
    if (!capacity != !max_events) return refuse(ctx, "kosk_monitor_reserve", "capacity and max_events are both at least 1, or both 0 (free)");
    if (monitor_reserve(*ctx->c, capacity, max_events)) { ctx->err = ctx->c->err; return -1; }
    return 0;
    GUARD_END
}

int kosk_monitor_level(const kosk_ctx *ctx, int *size, int *max_events, int *used, int *capacity, int *failed)
{
    if (!ctx) return -1;
    const KemRegistry *r = ctx->c->monitor;
    if (size) *size = r ? r->hist_size : 0;
    if (max_events) *max_events = r ? r->hist_max : 0;
    if (used) *used = r ? r->used : 0;
    if (capacity) *capacity = r ? r->capacity : 0;
    if (failed) *failed = r && r->mon_failed;
    return 0;
}

int kosk_monitor_feed(kosk_ctx *ctx, int n, const uint8_t *events, int *bad_index, int *reason)
{
    if (!ctx || n < 1 || !events) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    const KemRegistry *r = ctx->c->monitor;
    if (!r) return refuse(ctx, "kosk_monitor_feed", WHY_NO_MONITOR);
    if (r->mon_failed) return refuse(ctx, "kosk_monitor_feed", "the monitor has failed: a fed log was rejected (kosk_monitor_reserve starts a fresh replay)");
    if ((long)r->hist_size + n > (long)r->hist_max) return refuse(ctx, "kosk_monitor_feed", "monitor is full (kosk_monitor_reserve): nothing was changed");
    if (bad_index) *bad_index = -1;
    if (reason) *reason = KOSK_MONITOR_OK;
    const int rc = monitor_feed(*ctx->c, n, events, bad_index, reason);
    if (rc < 0) ctx->err = ctx->c->err;
    return rc;
    GUARD_END
}

int kosk_monitor_head(kosk_ctx *ctx, int size, uint8_t root[32], int *size_out)
{
    if (!ctx || !root) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    KemRegistry *r = ctx->c->monitor;
    if (!r) return refuse(ctx, "kosk_monitor_head", WHY_NO_MONITOR);
    if (size < 0) size = r->hist_size;
    if (size > r->hist_size) return refuse(ctx, "kosk_monitor_head", "size is above the current size of the monitor's history");
    if (reghist_head(*ctx->c, *r, size, root)) { ctx->err = ctx->c->err; return -1; }
    if (size_out) *size_out = size;
    return 0;
    GUARD_END
}

int kosk_monitor_roots(kosk_ctx *ctx, uint8_t slot_root[32], uint8_t sorted_root[32])
{
    if (!ctx) return -1;
    GUARD(ctx)
    ctx->clear_err();
    if (!ctx->c->monitor) return refuse(ctx, "kosk_monitor_roots", WHY_NO_MONITOR);
    if (monitor_roots(*ctx->c, slot_root, sorted_root)) { ctx->err = ctx->c->err; return -1; }
    return 0;
    GUARD_END
}

int kosk_monitor_read(kosk_ctx *ctx, int n, const int32_t *slots, uint8_t *state, uint8_t *h)
{
    if (!ctx || n < 1 || !slots || !state) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    const KemRegistry *r = ctx->c->monitor;
    if (!r) return refuse(ctx, "kosk_monitor_read", WHY_NO_MONITOR);
    for (int b = 0; b < n; b++)
        if (slots[b] < 0 || slots[b] >= r->capacity) return refuse(ctx, "kosk_monitor_read", "a slot id outside [0, capacity)");
    if (monitor_read(*ctx->c, n, slots, state, h)) { ctx->err = ctx->c->err; return -1; }
    return 0;
    GUARD_END
}

// ---- the relying party (kosk_relying.hip) ----
// the one root of a call on the host, wherever the caller keeps it
static int relying_root(kosk_ctx *ctx, const char *fn, const uint8_t *root, uint8_t (&out)[32])
{
    if (!is_device_pointer(root)) { memcpy(out, root, 32); return 0; }
    if (hipMemcpy(out, root, 32, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return refuse(ctx, fn, "copying the root to the host failed"); }
    return 0;
}

int kosk_regtree_check_paths(kosk_ctx *ctx, int n, int depth, const int32_t *slots, const uint8_t *state, const uint8_t *h, const uint8_t *paths, const uint8_t root[32], uint8_t *ok)
{
    if (!ctx) return -1;
    if (!slots || (!state && !h) || (depth > 0 && !paths) || !root || !ok) return refuse(ctx, __func__, "null pointer");
    if (n < 1) return refuse(ctx, __func__, "n must be at least 1");
    if (depth < 0 || depth > 31) return refuse(ctx, __func__, "depth outside 0..31");
    GUARD(ctx)
    ctx->clear_err();
    uint8_t r[32];
    if (relying_root(ctx, "kosk_regtree_check_paths", root, r)) return -1;
    const size_t rec = (size_t)depth * 32;
    return kem_chunks(ctx, n, [&](Ctx &c, int first, int count) {
        return regtree_check_paths(c, count, depth, slots + first, state ? state + first : nullptr, h ? h + (size_t)first * 32 : nullptr,
                                   paths ? paths + (size_t)first * rec : nullptr, r, ok + first);
    });
    GUARD_END
}

int kosk_regsort_check_proofs(kosk_ctx *ctx, int n, int depth, const uint8_t *x, const uint8_t *records, const uint8_t root[32], uint8_t *verdict)
{
    if (!ctx) return -1;
    if (!x || !records || !root || !verdict) return refuse(ctx, __func__, "null pointer");
    if (n < 1) return refuse(ctx, __func__, "n must be at least 1");
    if (depth < 0 || depth > 31) return refuse(ctx, __func__, "depth outside 0..31");
    GUARD(ctx)
    ctx->clear_err();
    uint8_t r[32];
    if (relying_root(ctx, "kosk_regsort_check_proofs", root, r)) return -1;
    const size_t rec = regsort::proof_bytes(depth);
    return kem_chunks(ctx, n, [&](Ctx &c, int first, int count) {
        return regsort_check_proofs(c, count, depth, x + (size_t)first * 32, records + (size_t)first * rec, r, verdict + first);
    });
    GUARD_END
}

int kosk_kem_enc_proven(kosk_ctx *ctx, int n, int depth, const uint8_t *pk, const int32_t *slots, const uint8_t *paths, const uint8_t root[32], const uint8_t *coins,
                        uint8_t *ct, uint8_t *ss, uint8_t *done)
{
    if (!ctx) return -1;
    if (!pk || !slots || (depth > 0 && !paths) || !root || !ct || !ss || !done) return refuse(ctx, __func__, "null pointer"); // before any coin is drawn
    if (n < 1) return refuse(ctx, __func__, "n must be at least 1");
    if (depth < 0 || depth > 31) return refuse(ctx, __func__, "depth outside 0..31");
    WGUARD(ctx)
    ctx->clear_err();
    uint8_t r[32];
    if (relying_root(ctx, "kosk_kem_enc_proven", root, r)) return -1;
    // coins are drawn for every position, whatever its path proves: the draw order does not depend on peer data
    std::vector<uint8_t> drawn;
    VecWiper<uint8_t> drawn_gone(drawn);
    const uint8_t *m = kem_coins(ctx, n, coins, drawn);
    const Params &P = ctx->c->P;
    const size_t ctb = kosk_ct_bytes(P.K), rec = (size_t)depth * 32;
    return kem_chunks(ctx, n, [&](Ctx &c, int first, int count) {
        return kem_enc_proven(c, count, depth, pk + (size_t)first * P.pk_bytes, slots + first, paths ? paths + (size_t)first * rec : nullptr, r,
                              m + (size_t)first * 32, ct + (size_t)first * ctb, ss + (size_t)first * 32, done + first);
    });
    WGUARD_END
}

// ---- signed heads, format kosk-headsig-v1 (kosk_headsig.hpp, kosk_headsig.hip) ----
static_assert((int)KOSK_HEADSIG_PUB_BYTES == (int)headsig::PUB_BYTES && (int)KOSK_HEADSIG_ITEMS_PER_BLOCK == (int)headsig::ITEMS_PER_BLOCK,
              "kosk_mi355x.h and kosk_headsig.hpp");
size_t kosk_headsig_sig_bytes(int height) { return headsig::sig_bytes(height); }
int kosk_headsig_statement(int kyber_k, const uint8_t root[32], int size, uint8_t out[56]) { return headsig::statement(kyber_k, root, size, out); }
int kosk_headsig_verify(const uint8_t pub[52], int kyber_k, const uint8_t root[32], int size, const uint8_t *sig)
{
    return headsig::verify(pub, kyber_k, root, size, sig);
}
int kosk_headsig_public_from_seed(int height, const uint8_t seed[32], const uint8_t id[16], uint8_t pub[52])
{
    return headsig::public_from_seed(height, seed, id, pub);
}

int kosk_registry_signer_reserve(kosk_ctx *ctx, int height, const uint8_t seed[32], const uint8_t id[16], uint8_t pub[52])
{
    if (!ctx) return -1;
    if (height && (!seed || !id || !pub)) return refuse(ctx, __func__, "null pointer");
    if (height < 0 || height > headsig::MAX_HEIGHT) return refuse(ctx, __func__, "height outside 0..24");
    GUARD(ctx)
    ctx->clear_err();
    const KemRegistry *r = ctx->c->registry;
    if (height && !r) return refuse(ctx, "kosk_registry_signer_reserve", WHY_NO_REGISTRY);
    if (height && !r->hist_max) return refuse(ctx, "kosk_registry_signer_reserve", WHY_NO_HISTORY);
    if (headsig_signer_reserve(*ctx->c, height, seed, id, pub)) { ctx->err = ctx->c->err; return -1; }
    return 0;
    GUARD_END
}

int kosk_registry_signer_level(kosk_ctx *ctx, int *height, int *has_seed)
{
    if (!ctx) return -1;
    if (height) *height = ctx->c->sg_height;
    if (has_seed) *has_seed = ctx->c->sg_height && ctx->c->sg_has_seed ? 1 : 0;
    return 0;
}

int kosk_registry_history_sign_head(kosk_ctx *ctx, int size, uint8_t *sig, uint8_t root[32], int *size_out)
{
    if (!ctx) return -1;
    if (!sig) return refuse(ctx, __func__, "null pointer");
    GUARD(ctx)
    ctx->clear_err();
    if (const char *why = history_refusal(ctx, size)) return refuse(ctx, "kosk_registry_history_sign_head", why);
    const Ctx &c = *ctx->c;
    if (!c.sg_height) return refuse(ctx, "kosk_registry_history_sign_head", "no signer is reserved (kosk_registry_signer_reserve)");
    if (!c.sg_has_seed) return refuse(ctx, "kosk_registry_history_sign_head", "seed was wiped (kosk_registry_signer_reserve with the same seed and id restores it)");
    if (((unsigned)size >> c.sg_height) != 0) return refuse(ctx, "kosk_registry_history_sign_head", "signer is exhausted: size is not below 2^height");
    if (headsig_sign_head(*ctx->c, size, sig, root)) { ctx->err = ctx->c->err; return -1; }
    if (size_out) *size_out = size;
    return 0;
    GUARD_END
}

int kosk_headsig_verify_heads(kosk_ctx *ctx, int n, const uint8_t pub[52], const uint8_t *roots, const int32_t *sizes, const uint8_t *sigs, uint8_t *ok)
{
    if (!ctx) return -1;
    if (!pub || !roots || !sizes || !sigs || !ok) return refuse(ctx, __func__, "null pointer");
    if (n < 1) return refuse(ctx, __func__, "n must be at least 1");
    GUARD(ctx)
    ctx->clear_err();
    uint8_t p[headsig::PUB_BYTES];
    if (!is_device_pointer(pub)) memcpy(p, pub, sizeof p);
    else if (hipMemcpy(p, pub, sizeof p, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); return refuse(ctx, "kosk_headsig_verify_heads", "copying the public key to the host failed"); }
    const size_t sb = headsig::sig_bytes((int)headsig::le32_in(p));
    if (!sb) return refuse(ctx, "kosk_headsig_verify_heads", "the public key's height is outside 1..24");
    return kem_chunks(ctx, n, [&](Ctx &c, int first, int count) {
        return headsig_verify_heads(c, count, p, roots + (size_t)first * 32, sizes + first, sigs + (size_t)first * sb, ok + first);
    });
    GUARD_END
}

// ---- existing keys: the witness from the secret key, and proofs for keys made elsewhere (kosk_witness_kernels.hip) ----
int kosk_witness_from_sk(kosk_ctx *ctx, int n, const uint8_t *sk, int16_t *se_out, uint8_t *ok)
{
    if (!ctx || n < 1 || n > ctx->max_batch || !sk || !ok) return bad_args(ctx, __func__);
    GUARD(ctx)
    const Params &P = ctx->c->P;
    return ctx->run(n, [&](Ctx &c, int first, int count) {
        return witness_from_sk(c, count, sk + (size_t)first * P.sk_bytes, se_out ? se_out + (size_t)first * 2 * P.K * 256 : nullptr, ok + first);
    });
    GUARD_END
}

// the randomness of a proof for an existing key: the draws of prepare_randomness, prepare_range_proof and prove in the reference's order
// and lengths (mlwe_prover.cpp:9, ss.cpp:5) at their places in the tape; the key generation's 64 bytes in front (kosk.cpp:12) are
// neither drawn nor read
static void draw_prover_tapes(const kosk_ctx *ctx, int n, std::vector<uint8_t> &drawn)
{
    const Params &P = ctx->c->P;
    drawn.assign((size_t)n * P.tape_bytes, 0);
    const Ctx &c0 = *ctx->c;
    for (int b = 0; b < n; b++) {
        uint8_t *tp = drawn.data() + (size_t)b * P.tape_bytes + 64;
        auto draw = [&](size_t len) { if (c0.rb) c0.rb(c0.rb_user, tp, len); else os_randombytes(tp, len); tp += len; };
        for (int i = 0; i < P.M; i++) draw(32);
        for (int i = 0; i < P.nfresh; i++) draw(302);
    }
}
static void resolve_for_keys(const kosk_ctx *ctx, int n, RandSrc &src)
{
    if (!src.seeded && !src.tapes) {
        draw_prover_tapes(ctx, n, src.drawn);
        src.tapes = src.drawn.data();
        src.tape_stride = ctx->c->P.tape_bytes;
    } else {
        src.resolve(ctx, n);
    }
}
static int stage_keys_at(Ctx &c, const Params &P, const RandSrc &src, int first, int count, const uint8_t *sk, uint8_t *ok)
{
    return stage_prover_keys(c, count, sk + (size_t)first * P.sk_bytes, src.seeded ? nullptr : src.tapes + (size_t)first * src.tape_stride, src.tape_stride,
                             src.seeded ? src.seeds + (size_t)first * src.seed_stride : nullptr, src.seed_stride, ok + first);
}
// The shared tail of the host-buffer calls on existing keys, chunk by chunk: the caller's staging step stage(c, first, count), which fills
// ok[first ...], then prove, fetch the images, and zero those of the rejected keys
static int prove_keys_chunks(kosk_ctx *ctx, int n, uint8_t *pi, const uint8_t *ok, const std::function<int(Ctx &, int, int)> &stage)
{
    const Params &P = ctx->c->P;
    const bool direct = copy_direct(ctx, pi, (size_t)n * P.proof_bytes);
    return run_chunks(ctx, n, [&](Ctx &c, int first, int count) {
        if (stage(c, first, count)) return -1;
        if (prove_at(c, first, count)) return -1;
        if (fetch_proofs_image(c, count, pi + (size_t)first * P.proof_bytes, direct)) return -1;
        for (int b = first; b < first + count; b++) // a rejected key's image (made from the zero witness) is not handed out
            if (!ok[b]) memset(pi + (size_t)b * P.proof_bytes, 0, P.proof_bytes);
        return 0;
    });
}
// the stride check of both twins: a tape call's against one tape, a seeded call's against one seed
static const char *key_stride_why(const kosk_ctx *ctx, bool seeded, const uint8_t *rand, size_t stride)
{
    if (!rand) return nullptr;
    if (seeded) return stride < SEED_BYTES ? WHY_SEED_STRIDE : nullptr;
    return stride < ctx->c->P.tape_bytes ? WHY_TAPE_STRIDE : nullptr;
}
static int stage_prover_keys_src(kosk_ctx *ctx, const char *fn, int n, const uint8_t *sk, bool seeded, const uint8_t *rand, size_t stride, uint8_t *ok)
{
    if (!ctx || n < 1 || n > ctx->max_batch || !sk || !ok) return bad_args(ctx, fn);
    if (const char *why = key_stride_why(ctx, seeded, rand, stride)) return refuse(ctx, fn, why);
    return guard(ctx, fn, [&]() -> int {
        const Params &P = ctx->c->P;
        RandSrc src = RandSrc::of(ctx, seeded, rand, stride);
        resolve_for_keys(ctx, n, src); // stateful callback: everything sequentially, in proof order
        return ctx->run(n, [&](Ctx &c, int first, int count) { return stage_keys_at(c, P, src, first, count, sk, ok); });
    });
}
static int prove_keys_src(kosk_ctx *ctx, const char *fn, int n, const uint8_t *sk, bool seeded, const uint8_t *rand, size_t stride, uint8_t *pi, uint8_t *ok)
{
    if (!ctx || n < 1 || !sk || !pi || !ok) return bad_args(ctx, fn);
    if (ctx->armed && n > ctx->armed) return refuse(ctx, fn, WHY_ARMED);
    if (const char *why = key_stride_why(ctx, seeded, rand, stride)) return refuse(ctx, fn, why);
    return guard(ctx, fn, [&]() -> int { return wiped_call(ctx, [&]() -> int {
        const Params &P = ctx->c->P;
        RandSrc src = RandSrc::of(ctx, seeded, rand, stride);
        resolve_for_keys(ctx, n, src);
        return prove_keys_chunks(ctx, n, pi, ok, [&](Ctx &c, int first, int count) { return stage_keys_at(c, P, src, first, count, sk, ok); });
    }); });
}
int kosk_stage_prover_keys(kosk_ctx *ctx, int n, const uint8_t *sk, const uint8_t *tapes, size_t tape_stride, uint8_t *ok)
{
    return stage_prover_keys_src(ctx, __func__, n, sk, false, tapes, tape_stride, ok);
}
int kosk_stage_prover_keys_seeded(kosk_ctx *ctx, int n, const uint8_t *sk, const uint8_t *seeds, size_t seed_stride, uint8_t *ok)
{
    return stage_prover_keys_src(ctx, __func__, n, sk, true, seeds, seed_stride, ok);
}
int kosk_prove_keys_batch(kosk_ctx *ctx, int n, const uint8_t *sk, const uint8_t *tapes, size_t tape_stride, uint8_t *pi, uint8_t *ok)
{
    return prove_keys_src(ctx, __func__, n, sk, false, tapes, tape_stride, pi, ok);
}
int kosk_prove_keys_seeded_batch(kosk_ctx *ctx, int n, const uint8_t *sk, const uint8_t *seeds, size_t seed_stride, uint8_t *pi, uint8_t *ok)
{
    return prove_keys_src(ctx, __func__, n, sk, true, seeds, seed_stride, pi, ok);
}

// ---- kosk-keyseed-v1: the randomness derived from the key itself.  Position b of the call hashes armed context b (the
// handle's device copy; chunks and sub-batches pass their offset on as for binding) and salt b
static int stage_derived_at(Ctx &c, const Params &P, int first, int count, const uint8_t *sk, const uint8_t *salts, size_t salt_stride, uint8_t *ok)
{
    const DerivedSrc src{salts ? salts + (size_t)first * salt_stride : nullptr, salt_stride};
    c.bind_first = first;
    return stage_prover_keys(c, count, sk + (size_t)first * P.sk_bytes, nullptr, 0, nullptr, 0, ok + first, &src);
}
int kosk_stage_prover_keys_derived(kosk_ctx *ctx, int n, const uint8_t *sk, const uint8_t *salts, size_t salt_stride, uint8_t *ok)
{
    if (!ctx || n < 1 || n > ctx->max_batch || !sk || !ok) return bad_args(ctx, __func__);
    ARMED_CHECK(ctx, n);
    if (salts && salt_stride < 32) return refuse(ctx, __func__, WHY_SALT_STRIDE);
    GUARD(ctx)
    const Params &P = ctx->c->P;
    return ctx->run(n, [&](Ctx &c, int first, int count) { return stage_derived_at(c, P, first, count, sk, salts, salt_stride, ok); });
    GUARD_END
}
int kosk_prove_keys_derived_batch(kosk_ctx *ctx, int n, const uint8_t *sk, const uint8_t *salts, size_t salt_stride, uint8_t *pi, uint8_t *ok)
{
    if (!ctx || n < 1 || !sk || !pi || !ok) return bad_args(ctx, __func__);
    ARMED_CHECK(ctx, n);
    if (salts && salt_stride < 32) return refuse(ctx, __func__, WHY_SALT_STRIDE);
    WGUARD(ctx)
    const Params &P = ctx->c->P;
    return prove_keys_chunks(ctx, n, pi, ok, [&](Ctx &c, int first, int count) { return stage_derived_at(c, P, first, count, sk, salts, salt_stride, ok); });
    WGUARD_END
}
int kosk_keyseed_device(kosk_ctx *ctx, int n, const uint8_t *sk, const uint8_t *contexts, size_t context_stride, const uint8_t *salts, size_t salt_stride,
                        uint8_t *d_seeds)
{
    if (!ctx || n < 1 || !sk || !d_seeds) return bad_args(ctx, __func__);
    WGUARD(ctx)
    ctx->clear_err();
    return keyseed_device(*ctx->c, n, sk, contexts, context_stride, salts, salt_stride, d_seeds);
    WGUARD_END
}

// ---- the offline bank (kosk_bank.hip): offline material banked ahead of the key, consumed exactly once ----
size_t kosk_bank_entry_bytes(int k) { Params p; return make_params(k, p) ? bank_entry_bytes(p) : 0; }
int kosk_tape_section(int k, int section, size_t *offset, size_t *size)
{
    Params p;
    if (!make_params(k, p) || !offset || !size) return -1;
    return tape_section(p, section, offset, size) ? 0 : -1;
}
static const char *const WHY_BANK_STREAMS = "needs streams = 1 (the bank belongs to one sub-context)";
static const char *const WHY_BANK_BOTH = "at most one of tapes / seeds";
// The randomness of a bank call: the caller's tapes (full format) or seeds, or, with neither, draws by the handle's entropy mode -- one seed
// per item, or the reference's draws for the sections `mask` of a tape in its order, into records that hold those sections only
struct BankRand {
    const uint8_t *tapes = nullptr, *seeds = nullptr;
    size_t tape_stride = 0, seed_stride = 0;
    bool compact = false; // drawn in tape mode: a record holds only the sections the call consumes
    std::vector<uint8_t> drawn;
    ~BankRand() { host_wipe_vec(drawn); }
    void resolve(const kosk_ctx *ctx, int n, unsigned mask)
    {
        if (tapes || seeds) return;
        const Ctx &c0 = *ctx->c;
        const Params &P = c0.P;
        if (c0.entropy_seed) {
            drawn.resize((size_t)n * SEED_BYTES);
            draw_seeds(c0, n, drawn.data());
            seeds = drawn.data();
            seed_stride = SEED_BYTES;
            return;
        }
        // compact records: exactly the sections of the mask back to back, every byte of them drawn (stage_tape_sections, compact)
        size_t rec = 0, off = 0, len = 0;
        for (int sec = 0; sec < 3; sec++)
            if ((mask >> sec & 1) && tape_section(P, sec, &off, &len)) rec += len;
        drawn.resize((size_t)n * rec);
        uint8_t *tp = drawn.data();
        auto draw = [&](size_t bytes) { if (c0.rb) c0.rb(c0.rb_user, tp, bytes); else os_randombytes(tp, bytes); tp += bytes; };
        for (int b = 0; b < n; b++) {
            if (mask >> TAPE_SEC_KEYSEED & 1) draw(64); // kosk.cpp:12
            if (mask >> TAPE_SEC_OFFLINE & 1) {
                for (int i = 0; i < P.M; i++) draw(32);                            // mlwe_prover.cpp:9
                for (int i = 0; i < 2 * P.M + 2 * P.K * P.E; i++) draw(302);       // ss.cpp:5
            }
            if (mask >> TAPE_SEC_ONLINE & 1) {
                tape_section(P, TAPE_SEC_ONLINE, &off, &len);
                for (size_t i = 0; i < len / 302; i++) draw(302);
            }
        }
        tapes = drawn.data();
        tape_stride = rec;
        compact = true;
    }
    const uint8_t *tapes_at(int first) const { return tapes ? tapes + (size_t)first * tape_stride : nullptr; }
    const uint8_t *seeds_at(int first) const { return seeds ? seeds + (size_t)first * seed_stride : nullptr; }
};
// the checks the four calls with randomness arguments share, behind bad_args: nullptr, or why the call is refused
static const char *bank_rand_why(const kosk_ctx *ctx, const uint8_t *tapes, size_t tape_stride, const uint8_t *seeds, size_t seed_stride)
{
    if (ctx->sub.size() > 1) return WHY_BANK_STREAMS;
    if (tapes && seeds) return WHY_BANK_BOTH;
    if (tapes && tape_stride < ctx->c->P.tape_bytes) return WHY_TAPE_STRIDE;
    if (seeds && seed_stride < SEED_BYTES) return WHY_SEED_STRIDE;
    return nullptr;
}
static const char *bank_level_why(const kosk_ctx *ctx, int n)
{
    if (ctx->c->bank_ready == 0) return "bank is empty (kosk_bank_fill makes entries)";
    return n > ctx->c->bank_ready ? "the bank holds fewer entries than this call has proofs (kosk_bank_level)" : nullptr;
}
int kosk_bank_reserve(kosk_ctx *ctx, int capacity)
{
    if (!ctx) return -1;
    if (capacity < 0) return refuse(ctx, __func__, "the capacity cannot be negative");
    if (ctx->sub.size() > 1) return refuse(ctx, __func__, WHY_BANK_STREAMS);
    if (ctx->c->bank_ready) return refuse(ctx, __func__, "the bank is not empty: its entries are consumed, or wiped by kosk_wipe_secrets, before it is reserved again");
    GUARD(ctx)
    ctx->clear_err();
    return bank_reserve(*ctx->c, capacity);
    GUARD_END
}
int kosk_bank_level(const kosk_ctx *ctx, int *ready, int *capacity)
{
    if (!ctx || !ready || !capacity) return -1;
    *ready = ctx->c->bank_ready;
    *capacity = ctx->c->bank_cap;
    return 0;
}
int kosk_bank_fill(kosk_ctx *ctx, int n, const uint8_t *tapes, size_t tape_stride, const uint8_t *seeds, size_t seed_stride)
{
    if (!ctx || n < 1) return bad_args(ctx, __func__);
    if (const char *why = bank_rand_why(ctx, tapes, tape_stride, seeds, seed_stride)) return refuse(ctx, __func__, why);
    if (n > ctx->c->bank_cap - ctx->c->bank_ready) return refuse(ctx, __func__, "the bank has no room for this many entries (kosk_bank_reserve, kosk_bank_level)");
    WGUARD(ctx)
    BankRand r;
    r.tapes = tapes; r.tape_stride = tape_stride; r.seeds = seeds; r.seed_stride = seed_stride;
    r.resolve(ctx, n, 1u << TAPE_SEC_OFFLINE); // stateful callback: everything sequentially, in entry order
    return serial_chunks(ctx, n, [&](Ctx &c, int first, int count) { return bank_fill(c, count, r.tapes_at(first), r.tape_stride, r.seeds_at(first), r.seed_stride, r.compact); });
    WGUARD_END
}
int kosk_stage_prover_keys_banked(kosk_ctx *ctx, int n, const uint8_t *sk, const uint8_t *tapes, size_t tape_stride, const uint8_t *seeds, size_t seed_stride,
                                  uint8_t *ok)
{
    if (!ctx || n < 1 || n > ctx->max_batch || !sk || !ok) return bad_args(ctx, __func__);
    if (const char *why = bank_rand_why(ctx, tapes, tape_stride, seeds, seed_stride)) return refuse(ctx, __func__, why);
    if (const char *why = bank_level_why(ctx, n)) return refuse(ctx, __func__, why);
    GUARD(ctx)
    ctx->clear_err();
    BankRand r;
    r.tapes = tapes; r.tape_stride = tape_stride; r.seeds = seeds; r.seed_stride = seed_stride;
    r.resolve(ctx, n, 1u << TAPE_SEC_ONLINE);
    return stage_prover_keys_banked(*ctx->c, n, sk, r.tapes, r.tape_stride, r.seeds, r.seed_stride, ok, r.compact);
    GUARD_END
}
int kosk_prove_keys_banked_batch(kosk_ctx *ctx, int n, const uint8_t *sk, const uint8_t *tapes, size_t tape_stride, const uint8_t *seeds, size_t seed_stride,
                                 uint8_t *pi, uint8_t *ok)
{
    if (!ctx || n < 1 || !sk || !pi || !ok) return bad_args(ctx, __func__);
    ARMED_CHECK(ctx, n);
    if (const char *why = bank_rand_why(ctx, tapes, tape_stride, seeds, seed_stride)) return refuse(ctx, __func__, why);
    if (const char *why = bank_level_why(ctx, n)) return refuse(ctx, __func__, why);
    WGUARD(ctx)
    const Params &P = ctx->c->P;
    BankRand r;
    r.tapes = tapes; r.tape_stride = tape_stride; r.seeds = seeds; r.seed_stride = seed_stride;
    r.resolve(ctx, n, 1u << TAPE_SEC_ONLINE);
    const bool direct = copy_direct(ctx, pi, (size_t)n * P.proof_bytes);
    // proof b of the call takes the b-th oldest entry: the chunks run one after the other on the bank's sub-context
    return serial_chunks(ctx, n, [&](Ctx &c, int first, int count) {
        if (stage_prover_keys_banked(c, count, sk + (size_t)first * P.sk_bytes, r.tapes_at(first), r.tape_stride, r.seeds_at(first), r.seed_stride, ok + first, r.compact)) return -1;
        if (prove_at(c, first, count)) return -1;
        if (fetch_proofs_image(c, count, pi + (size_t)first * P.proof_bytes, direct)) return -1;
        for (int b = first; b < first + count; b++) // a rejected key's image (made from the zero witness) is not handed out
            if (!ok[b]) memset(pi + (size_t)b * P.proof_bytes, 0, P.proof_bytes);
        return 0;
    });
    WGUARD_END
}
int kosk_verifiable_keygen_banked_batch(kosk_ctx *ctx, int n, const uint8_t *tapes, size_t tape_stride, const uint8_t *seeds, size_t seed_stride, uint8_t *pk,
                                        uint8_t *sk, uint8_t *pi)
{
    if (!ctx || n < 1 || !pk || !sk || !pi) return bad_args(ctx, __func__);
    ARMED_CHECK(ctx, n);
    if (const char *why = bank_rand_why(ctx, tapes, tape_stride, seeds, seed_stride)) return refuse(ctx, __func__, why);
    if (const char *why = bank_level_why(ctx, n)) return refuse(ctx, __func__, why);
    WGUARD(ctx)
    const Params &P = ctx->c->P;
    BankRand r;
    r.tapes = tapes; r.tape_stride = tape_stride; r.seeds = seeds; r.seed_stride = seed_stride;
    const unsigned mask = 1u << TAPE_SEC_KEYSEED | 1u << TAPE_SEC_ONLINE;
    r.resolve(ctx, n, mask); // the key generation's 64 bytes first, then the online draws
    const bool direct = copy_direct(ctx, pi, (size_t)n * P.proof_bytes);
    return serial_chunks(ctx, n, [&](Ctx &c, int first, int count) {
        KeygenIn kg{r.tapes_at(first), r.tape_stride, pk + (size_t)first * P.pk_bytes, sk + (size_t)first * P.sk_bytes};
        if (r.seeds) { kg.seeds = r.seeds_at(first); kg.seed_stride = r.seed_stride; }
        kg.sections = mask;
        kg.sections_compact = r.compact;
        if (bank_take(c, count)) return -1;
        c.bind_first = first;
        if (prove_resident(c, count, true, &kg)) return -1;
        return fetch_proofs_image(c, count, pi + (size_t)first * P.proof_bytes, direct);
    });
    WGUARD_END
}
// diagnostic (tools/bank_rate.py): k_bank_put / k_bank_take of n entries on an empty bank against the runtime's own D2D copies and fill
int kosk_bank_timing(kosk_ctx *ctx, int n, int reps, double *put_ms, double *take_ms, double *copy_ms, double *copy_fill_ms, size_t *bytes)
{
    if (!ctx || n < 1 || reps < 1 || !put_ms || !take_ms || !copy_ms || !copy_fill_ms) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    return bank_timing(*ctx->c, n, reps, put_ms, take_ms, copy_ms, copy_fill_ms, bytes);
    GUARD_END
}

void *kosk_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (!bytes || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}
void kosk_host_free(void *p)
{
    if (p && hipHostFree(p) != hipSuccess) (void)hipGetLastError();
}

// ---- erasure (kosk_wipe.hip) ----
int kosk_wipe_secrets(kosk_ctx *ctx)
{
    if (!ctx) return -1;
    GUARD(ctx)
    ctx->clear_err();
    return wipe_handle(ctx);
    GUARD_END
}
int kosk_set_wipe(kosk_ctx *ctx, int mode)
{
    if (!ctx) return -1;
    if (mode != KOSK_WIPE_OFF && mode != KOSK_WIPE_CALL) return bad_args(ctx, __func__);
    ctx->wipe_mode = mode;
    return 0;
}
int kosk_secret_scan(kosk_ctx *ctx, const uint8_t *needle, size_t len, long *hits)
{
    if (!ctx || !needle || !hits || len < 16 || len > 64) return -1;
    GUARD(ctx)
    ctx->clear_err();
    Ctx &c = *ctx->c;
    HIPCHK_C(hipSetDevice(c.device));
    // the scan's own scratch, outside the inventory: the needle's device copy and the block counters, and their page-locked mirror
    uint8_t *d = nullptr;
    unsigned long long *h_slots = nullptr;
    const size_t slot_bytes = sizeof(unsigned long long) * SCAN_SLOT_COUNT;
    HIPCHK_C(hipMalloc(reinterpret_cast<void **>(&d), 64 + slot_bytes));
    // however the call ends, the needle's copy is cleared before it is freed (by the runtime's fill: kosk_path_count id 18 counts
    // wipes, not scans)
    struct Free {
        uint8_t *d; unsigned long long *&h; hipStream_t st;
        ~Free()
        {
            if (hipMemsetAsync(d, 0, 64, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) (void)hipGetLastError();
            (void)hipFree(d);
            if (h) (void)hipHostFree(h);
        }
    } fr{d, h_slots, c.stream};
    HIPCHK_C(hipHostMalloc(reinterpret_cast<void **>(&h_slots), slot_bytes, hipHostMallocDefault));
    HIPCHK_C(hipMemcpyAsync(d, needle, len, hipMemcpyHostToDevice, c.stream));
    HIPCHK_C(stream_sync(c));
    long total = 0;
    int rc = 0;
    for (Ctx *x : ctx->sub) {
        long n = 0;
        if (secret_scan(*x, needle, len, d, reinterpret_cast<unsigned long long *>(d + 64), h_slots, &n)) { ctx->err = x->err; rc = -1; break; }
        total += n;
    }
    if (rc) return -1;
    *hits = total;
    return 0;
    GUARD_END
}
// kernel level (tests): k_wipe on the caller's own device memory, region i = [d_ptrs[i], d_ptrs[i] + bytes[i]); synchronised
int kosk_wipe_device(kosk_ctx *ctx, int nregions, void *const *d_ptrs, const size_t *bytes)
{
    if (!ctx || nregions < 0 || (nregions && (!d_ptrs || !bytes))) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    Ctx &c = *ctx->c;
    HIPCHK_C(hipSetDevice(c.device));
    std::vector<WipeRegion> regs;
    for (int i = 0; i < nregions; i++) {
        if (!bytes[i]) continue;
        if (!d_ptrs[i] || !is_device_pointer(d_ptrs[i])) return bad_args(ctx, "kosk_wipe_device");
        regs.push_back(WipeRegion{static_cast<uint8_t *>(d_ptrs[i]), bytes[i], 0, 1});
    }
    if (launch_wipe(c, regs.data(), (int)regs.size())) return -1;
    HIPCHK_C(stream_sync(c));
    return 0;
    GUARD_END
}

// diagnostic (tools/wipe_rate.py): `reps` wipes of sub-context 0's secret HBM regions by k_wipe, then the same regions by the runtime's
// own fills (one hipMemsetAsync / hipMemset2DAsync per region), each between two events on the handle's stream
int kosk_wipe_timing(kosk_ctx *ctx, int reps, double *wipe_ms, double *memset_ms, size_t *bytes, int *regions)
{
    if (!ctx || reps < 1 || !wipe_ms || !memset_ms) return bad_args(ctx, __func__);
    GUARD(ctx)
    ctx->clear_err();
    Ctx &c = *ctx->c;
    HIPCHK_C(hipSetDevice(c.device));
    std::vector<WipeRegion> regs;
    wipe_regions_list(c, regs);
    size_t total = 0;
    for (const WipeRegion &r : regs) total += r.bytes * r.count;
    if (bytes) *bytes = total;
    if (regions) *regions = (int)regs.size();
    hipEvent_t ev[2] = {nullptr, nullptr};
    struct Ev { hipEvent_t *e; ~Ev() { for (int i = 0; i < 2; i++) if (e[i]) (void)hipEventDestroy(e[i]); } } evs{ev};
    HIPCHK_C(hipEventCreate(&ev[0]));
    HIPCHK_C(hipEventCreate(&ev[1]));
    float ms = 0;
    if (wipe_secrets(c)) return -1; // warm: first launch, and whatever staged inputs there were are gone either way
    HIPCHK_C(hipEventRecord(ev[0], c.stream));
    for (int i = 0; i < reps; i++)
        if (launch_wipe(c, regs.data(), (int)regs.size())) return -1;
    HIPCHK_C(hipEventRecord(ev[1], c.stream));
    HIPCHK_C(hipEventSynchronize(ev[1]));
    HIPCHK_C(hipEventElapsedTime(&ms, ev[0], ev[1]));
    *wipe_ms = ms / reps;
    HIPCHK_C(hipEventRecord(ev[0], c.stream));
    for (int i = 0; i < reps; i++)
        for (const WipeRegion &r : regs) {
            if (r.count == 1) HIPCHK_C(hipMemsetAsync(r.p, 0, r.bytes, c.stream));
            else HIPCHK_C(hipMemset2DAsync(r.p, r.stride, 0, r.bytes, r.count, c.stream));
        }
    HIPCHK_C(hipEventRecord(ev[1], c.stream));
    HIPCHK_C(hipEventSynchronize(ev[1]));
    HIPCHK_C(hipEventElapsedTime(&ms, ev[0], ev[1]));
    *memset_ms = ms / reps;
    return 0;
    GUARD_END
}

int kosk_path_count(const kosk_ctx *ctx, int id, long *count)
{
    if (!ctx || id < 0 || id >= PATH_COUNT || !count) return bad_args(ctx, __func__);
    long v = 0;
    for (const Ctx *c : ctx->sub) v += c->path_n[id];
    *count = v;
    return 0;
}
int kosk_host_threads(const kosk_ctx *ctx) { return ctx ? ctx->c->nthreads : -1; }

int kosk_phase_seconds(const kosk_ctx *ctx, double *out, int n)
{
    if (!ctx || !out) return -1;
    for (int i = 0; i < n && i < PH_COUNT; i++) out[i] = ctx->c->phase_sec[i];
    return 0;
}

int kosk_profile_enable(kosk_ctx *ctx, int on)
{
    if (!ctx) return -1;
    GUARD(ctx)
    for (Ctx *cp : ctx->sub) {
        Ctx &c = *cp;
        c.prof_on = on < 0 ? 0 : (on > 2 ? 2 : on);
        for (int i = 0; i < PR_COUNT; i++) { c.prof_ms[i] = 0; c.prof_n[i] = 0; c.prof_units[i] = 0; c.prof_used[i] = false; }
    }
    return 0;
    GUARD_END
}
int kosk_profile_read(const kosk_ctx *ctx, int id, double *total_ms, long *launches)
{
    if (!ctx || id < 0 || id >= PR_COUNT) return bad_args(ctx, __func__);
    double ms = 0;
    long cnt = 0;
    for (const Ctx *c : ctx->sub) { ms += c->prof_ms[id]; cnt += c->prof_n[id]; }
    if (total_ms) *total_ms = ms;
    if (launches) *launches = cnt;
    return 0;
}

int kosk_profile_read_units(const kosk_ctx *ctx, int id, double *total_ms, long *launches, long *proofs)
{
    if (!ctx || id < 0 || id >= PR_COUNT) return bad_args(ctx, __func__);
    double ms = 0;
    long cnt = 0, units = 0;
    for (const Ctx *c : ctx->sub) { ms += c->prof_ms[id]; cnt += c->prof_n[id]; units += c->prof_units[id]; }
    if (total_ms) *total_ms = ms;
    if (launches) *launches = cnt;
    if (proofs) *proofs = units;
    return 0;
}
int kosk_combine_stats(const kosk_ctx *ctx, long *calls, long *members)
{
    if (!ctx) return -1;
    if (calls) *calls = ctx->merged_calls;
    if (members) *members = ctx->merged_members;
    return 0;
}

int kosk_stream_timer_start(kosk_ctx *ctx)
{
    if (!ctx) return -1;
    GUARD(ctx)
    Ctx &c = *ctx->c;
    ctx->clear_err();
    HIPCHK_C(hipSetDevice(c.device));
    if (!c.timer_ev[0]) { HIPCHK_C(hipEventCreate(&c.timer_ev[0])); HIPCHK_C(hipEventCreate(&c.timer_ev[1])); }
    HIPCHK_C(hipEventRecord(c.timer_ev[0], c.stream));
    return 0;
    GUARD_END
}
int kosk_stream_timer_stop(kosk_ctx *ctx, double *ms)
{
    if (!ctx || !ctx->c->timer_ev[0]) return bad_args(ctx, __func__);
    GUARD(ctx)
    Ctx &c = *ctx->c;
    ctx->clear_err();
    HIPCHK_C(hipSetDevice(c.device));
    HIPCHK_C(hipEventRecord(c.timer_ev[1], c.stream));
    HIPCHK_C(hipEventSynchronize(c.timer_ev[1]));
    float f = 0;
    HIPCHK_C(hipEventElapsedTime(&f, c.timer_ev[0], c.timer_ev[1]));
    if (ms) *ms = f;
    return 0;
    GUARD_END
}

int kosk_device_synchronize(kosk_ctx *ctx)
{
    if (!ctx) return -1;
    GUARD(ctx)
    ctx->clear_err();
    for (Ctx *cp : ctx->sub) {
        Ctx &c = *cp;
        HIPCHK_C(hipSetDevice(c.device));
        HIPCHK_C(hipStreamSynchronize(c.stream));
    }
    return 0;
    GUARD_END
}
int kosk_streams(const kosk_ctx *ctx) { return ctx ? (int)ctx->sub.size() : -1; }

int kosk_resident_proofs(kosk_ctx *ctx, void **d_proofs, size_t *stride)
{
    if (!ctx) return -1;
    GUARD(ctx)
    if (ctx->sub.size() > 1) return refuse(ctx, nullptr, "kosk_resident_proofs needs streams = 1 (sub-batches keep separate images)");
    if (d_proofs) *d_proofs = ctx->c->d_proof;
    if (stride) *stride = ctx->c->image_stride;
    return 0;
    GUARD_END
}

// ---- kernel-level entry points -------------------------------------------------

int kosk_sha3_256_batch(kosk_ctx *ctx, const uint8_t *d_in, size_t in_stride, size_t inlen, uint8_t *d_out, int n)
{
    if (!ctx) return -1;
    GUARD(ctx)
    Ctx &c = *ctx->c;
    ctx->clear_err();
    HIPCHK_C(hipSetDevice(c.device));
    HIPCHK_C(launch_sha3_msgs(d_in, in_stride, (int)inlen, d_out, 32, 32, n, 0x06, c.stream));
    return 0;
    GUARD_END
}
int kosk_shake256_batch(kosk_ctx *ctx, const uint8_t *d_in, size_t in_stride, size_t inlen, uint8_t *d_out, size_t outlen, int n)
{
    if (!ctx) return -1;
    GUARD(ctx)
    Ctx &c = *ctx->c;
    ctx->clear_err();
    HIPCHK_C(hipSetDevice(c.device));
    HIPCHK_C(launch_sha3_msgs(d_in, in_stride, (int)inlen, d_out, outlen, (int)outlen, n, 0x1F, c.stream));
    return 0;
    GUARD_END
}

int kosk_sha3_256_batch_pair(kosk_ctx *ctx, const uint8_t *d_in, size_t in_stride, size_t inlen, uint8_t *d_out, int n)
{
    if (!ctx) return -1;
    GUARD(ctx)
    Ctx &c = *ctx->c;
    ctx->clear_err();
    HIPCHK_C(hipSetDevice(c.device));
    HIPCHK_C(launch_sha3_msgs_pair(d_in, in_stride, (int)inlen, d_out, 32, 32, n, 0x06, c.stream));
    return 0;
    GUARD_END
}

// sha3_256 of n LONG messages, one wave per message (the sponge of the device Fiat-Shamir rounds, kosk_fs_kernels.hip)
int kosk_sha3_256_batch_wave(kosk_ctx *ctx, const uint8_t *d_in, size_t in_stride, size_t inlen, uint8_t *d_out, int n)
{
    if (!ctx || !d_in || !d_out || n < 1 || inlen > (size_t)1 << 30 || (reinterpret_cast<uintptr_t>(d_in) & 7) || (in_stride & 7)) return bad_args(ctx, __func__);
    GUARD(ctx)
    Ctx &c = *ctx->c;
    ctx->clear_err();
    HIPCHK_C(hipSetDevice(c.device));
    FsArgs fa{};
    fa.in = d_in; fa.in_stride = in_stride; fa.len = (int)inlen; fa.out_digest = d_out;
    HIPCHK_C(launch_fs_chain(fa, FS_DIGEST, n, c.stream));
    return 0;
    GUARD_END
}
// kosk_fs_alpha / kosk_fs_opened for n digest tables in HBM (what the device Fiat-Shamir mode of a handle runs inside its calls)
int kosk_fs_alpha_device(kosk_ctx *ctx, const uint8_t *d_tables, size_t table_stride, int n, uint16_t *d_alpha, uint8_t *d_h1)
{
    if (!ctx || !d_tables || !d_alpha || n < 1 || (reinterpret_cast<uintptr_t>(d_tables) & 7) || (table_stride & 7)) return bad_args(ctx, __func__);
    GUARD(ctx)
    Ctx &c = *ctx->c;
    ctx->clear_err();
    HIPCHK_C(hipSetDevice(c.device));
    FsArgs fa{};
    fa.in = d_tables; fa.in_stride = table_stride; fa.len = NPARTY * 32; fa.out_digest = d_h1;
    fa.alpha = d_alpha; fa.alpha_stride = 80; fa.J = c.P.J;
    HIPCHK_C(launch_fs_chain(fa, FS_ALPHA, n, c.stream));
    return 0;
    GUARD_END
}
int kosk_fs_opened_device(kosk_ctx *ctx, const uint8_t *d_tables, size_t table_stride, int n, uint16_t *d_sel, uint16_t *d_rest, int sel_stride, uint8_t *d_ch)
{
    if (!ctx || !d_tables || !d_sel || !d_rest || n < 1 || sel_stride < NREST || sel_stride < SEL_OPOS + NOPEN ||
        (reinterpret_cast<uintptr_t>(d_tables) & 7) || (table_stride & 7)) return bad_args(ctx, __func__);
    GUARD(ctx)
    Ctx &c = *ctx->c;
    ctx->clear_err();
    HIPCHK_C(hipSetDevice(c.device));
    FsArgs fa{};
    fa.in = d_tables; fa.in_stride = table_stride; fa.len = NPARTY * 32; fa.out_digest = d_ch;
    fa.I = d_sel; fa.rest = d_rest; fa.sel_stride = sel_stride;
    if (c.force_n > 0) { fa.cand = c.force_d; fa.cand_n = c.force_n; } // tests: tables b < force_n take the handle's candidate lists
    HIPCHK_C(launch_fs_chain(fa, FS_OPENED, n, c.stream));
    return 0;
    GUARD_END
}

// ---- kosk-bind-v1: the binding values and the bound chains as kernel-level entry points
int kosk_bind_device(kosk_ctx *ctx, int n, const uint8_t *pk, const uint8_t *contexts, size_t context_stride, uint8_t *d_out)
{
    if (!ctx || n < 1 || !pk || !contexts || !d_out || context_stride < 32 || (reinterpret_cast<uintptr_t>(d_out) & 7)) return bad_args(ctx, __func__);
    GUARD(ctx)
    Ctx &c = *ctx->c;
    ctx->clear_err();
    HIPCHK_C(hipSetDevice(c.device));
    // pk (n records of pk_bytes) and contexts, host or device memory, into aligned device staging: the kernel loads 8 bytes at a time
    const size_t pkb = c.P.pk_bytes;
    uint8_t *stage = nullptr;
    HIPCHK_C(hipMalloc(reinterpret_cast<void **>(&stage), (size_t)n * (pkb + 32)));
    struct Free { uint8_t *p; ~Free() { (void)hipFree(p); } } fr{stage};
    uint8_t *d_ctx = stage + (size_t)n * pkb;
    HIPCHK_C(hipMemcpyAsync(stage, pk, (size_t)n * pkb, is_device_pointer(pk) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c.stream));
    HIPCHK_C(hipMemcpy2DAsync(d_ctx, 32, contexts, context_stride, 32, (size_t)n, is_device_pointer(contexts) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c.stream));
    BindArgs ba{};
    ba.pk = stage; ba.pk_stride = pkb; ba.pk_bytes = (int)pkb; ba.K = c.P.K; ba.contexts = d_ctx; ba.out = d_out;
    HIPCHK_C(launch_bind_values(ba, n, c.stream));
    HIPCHK_C(stream_sync(c)); // the staging buffer goes with the call
    return 0;
    GUARD_END
}
int kosk_fs_alpha_bound_device(kosk_ctx *ctx, const uint8_t *d_tables, size_t table_stride, int n, const uint8_t *d_bind, uint16_t *d_alpha, uint8_t *d_h1)
{
    if (!ctx || !d_tables || !d_alpha || !d_bind || n < 1 || (reinterpret_cast<uintptr_t>(d_tables) & 7) || (table_stride & 7) ||
        (reinterpret_cast<uintptr_t>(d_bind) & 7)) return bad_args(ctx, __func__);
    GUARD(ctx)
    Ctx &c = *ctx->c;
    ctx->clear_err();
    HIPCHK_C(hipSetDevice(c.device));
    FsArgs fa{};
    fa.in = d_tables; fa.in_stride = table_stride; fa.len = NPARTY * 32; fa.out_digest = d_h1;
    fa.alpha = d_alpha; fa.alpha_stride = 80; fa.J = c.P.J; fa.bind = d_bind;
    HIPCHK_C(launch_fs_chain(fa, FS_ALPHA, n, c.stream));
    return 0;
    GUARD_END
}
int kosk_fs_opened_bound_device(kosk_ctx *ctx, const uint8_t *d_tables, size_t table_stride, int n, const uint8_t *d_bind, uint16_t *d_sel, uint16_t *d_rest,
                                int sel_stride, uint8_t *d_ch)
{
    if (!ctx || !d_tables || !d_sel || !d_rest || !d_bind || n < 1 || sel_stride < NREST || sel_stride < SEL_OPOS + NOPEN ||
        (reinterpret_cast<uintptr_t>(d_tables) & 7) || (table_stride & 7) || (reinterpret_cast<uintptr_t>(d_bind) & 7)) return bad_args(ctx, __func__);
    GUARD(ctx)
    Ctx &c = *ctx->c;
    ctx->clear_err();
    HIPCHK_C(hipSetDevice(c.device));
    FsArgs fa{};
    fa.in = d_tables; fa.in_stride = table_stride; fa.len = NPARTY * 32; fa.out_digest = d_ch;
    fa.I = d_sel; fa.rest = d_rest; fa.sel_stride = sel_stride; fa.bind = d_bind;
    if (c.force_n > 0) { fa.cand = c.force_d; fa.cand_n = c.force_n; } // tests: tables b < force_n take the handle's candidate lists
    HIPCHK_C(launch_fs_chain(fa, FS_OPENED, n, c.stream));
    return 0;
    GUARD_END
}

int kosk_commit_hash_lanes(kosk_ctx *ctx, const uint16_t *d_rows, size_t row_stride, int n_lanes,
                           const uint8_t *d_prefix, int with_prefix, uint8_t *d_out)
{
    if (!ctx) return -1;
    GUARD(ctx)
    Ctx &c = *ctx->c;
    ctx->clear_err();
    HIPCHK_C(hipSetDevice(c.device));
    HashArgs ha{};
    ha.rows = d_rows;
    ha.group_stride = 0;
    ha.row_stride = (int)row_stride;
    ha.col_off = 0;
    ha.lanes_per_group = n_lanes;
    ha.prefix = d_prefix;
    ha.out = d_out;
    ha.out_lanes_per_group = n_lanes;
    int variant = 0;
    HIPCHK_C(launch_commit_hash(ha, 1, c.P.K, with_prefix != 0, c.stream, &variant));
    c.path_n[(variant & 1) ? PATH_HASH_DMA : PATH_HASH_PLAIN]++;
    return 0;
    GUARD_END
}

int kosk_ntt256_batch(kosk_ctx *ctx, const int16_t *d_in, int16_t *d_out, int n)
{
    if (!ctx) return -1;
    GUARD(ctx)
    Ctx &c = *ctx->c;
    ctx->clear_err();
    HIPCHK_C(hipSetDevice(c.device));
    NttArgs na{};
    na.in = d_in;
    na.out = d_out;
    na.npg = n;
    na.npoly = n;
    na.out_canonical = 0;
    HIPCHK_C(launch_ntt(na, c.stream));
    return 0;
    GUARD_END
}

int kosk_lagrange_expand(kosk_ctx *ctx, const uint16_t *d_y407, uint16_t *d_shares, int n)
{
    if (!ctx) return -1;
    GUARD(ctx)
    Ctx &c = *ctx->c;
    ctx->clear_err();
    HIPCHK_C(hipSetDevice(c.device));
    const int cap = c.own_batch * c.rm.nrows; // the row matrix doubles as scratch (this handle's own block of it)
    for (int done = 0; done < n;) {
        const int m = (n - done) < cap ? (n - done) : cap;
        HIPCHK_C(launch_rows_copy(d_y407 + (size_t)done * XLEN, XLEN, c.d_P, RS, XLEN, m, c.stream));
        const GemmSrc gs{c.d_P, 0, nullptr, RS, 0, 0}; // caller data: folded while converted
        const GemmDst gd{c.d_P, 0, nullptr, RS, EXP_OFF};
        if (gemm_modq(c, c.t_expand, gs, gd, m, 1)) return -1;
        HIPCHK_C(launch_rows_copy(c.d_P + NSEC, RS, d_shares + (size_t)done * NPARTY, NPARTY, NPARTY, m, c.stream));
        done += m;
    }
    return 0;
    GUARD_END
}

int kosk_recon_secrets(kosk_ctx *ctx, const uint16_t *d_shares, uint16_t *d_secrets, int n, int two_d)
{
    if (!ctx) return -1;
    GUARD(ctx)
    Ctx &c = *ctx->c;
    ctx->clear_err();
    HIPCHK_C(hipSetDevice(c.device));
    const GemmTable &t = two_d ? c.t_recon_2d : c.t_recon_d;
    const int cap = c.own_batch * c.rm.nrows;
    for (int done = 0; done < n;) {
        const int m = (n - done) < cap ? (n - done) : cap;
        HIPCHK_C(launch_rows_copy(d_shares + (size_t)done * NPARTY, NPARTY, c.d_P + NSEC, RS, NPARTY, m, c.stream));
        const GemmSrc gs{c.d_P, 0, nullptr, RS, NSEC, 0};
        const GemmDst gd{c.d_P, 0, nullptr, RS, 0};
        if (gemm_modq(c, t, gs, gd, m, 1)) return -1;
        HIPCHK_C(launch_rows_copy(c.d_P, RS, d_secrets + (size_t)done * NSEC, NSEC, NSEC, m, c.stream));
        done += m;
    }
    return 0;
    GUARD_END
}

// ---- host-only entry points -----------------------------------------------------

int kosk_keygen(int kyber_k, const uint8_t seed64[64], uint8_t *pk, uint8_t *sk, int16_t *A, int16_t *s, int16_t *e, int16_t *t)
{
    Params P;
    if (!make_params(kyber_k, P) || !seed64 || !pk || !sk) return -1;
    return guard(static_cast<const kosk_ctx *>(nullptr), __func__, [&]() -> int {
    std::unique_ptr<HostKey> key(new HostKey());
    struct Gone { HostKey *k; ~Gone() { host_wipe(k, sizeof(HostKey)); } } gone{key.get()}; // s, e: not back to the heap readable, however this ends
    host_keygen(P, seed64, pk, sk, *key);
    const int K = P.K;
    if (A) memcpy(A, key->A, sizeof(int16_t) * K * K * 256);
    if (s) memcpy(s, key->se, sizeof(int16_t) * K * 256);
    if (e) memcpy(e, key->se + K * 256, sizeof(int16_t) * K * 256);
    if (t) memcpy(t, key->t, sizeof(int16_t) * K * 256);
    return 0;
    GUARD_END
}

int kosk_fs_alpha(int kyber_k, const uint8_t *tcomm_all, uint16_t *alpha)
{
    Params P;
    if (!make_params(kyber_k, P) || !tcomm_all || !alpha) return -1;
    return guard(static_cast<const kosk_ctx *>(nullptr), __func__, [&]() -> int {
    fs_alpha(P, tcomm_all, alpha);
    return 0;
    GUARD_END
}

int kosk_fs_opened(const uint8_t *digests_all, uint16_t *I, uint16_t *rest)
{
    if (!digests_all || !I || !rest) return -1;
    return guard(static_cast<const kosk_ctx *>(nullptr), __func__, [&]() -> int {
    fs_opened(digests_all, I, rest);
    return 0;
    GUARD_END
}

int kosk_bind_value(int kyber_k, const uint8_t *pk, const uint8_t context[32], uint8_t out[32])
{
    Params P;
    if (!make_params(kyber_k, P) || !pk || !context || !out) return -1;
    return guard(static_cast<const kosk_ctx *>(nullptr), __func__, [&]() -> int {
    bind_value(P, pk, context, out);
    return 0;
    GUARD_END
}
int kosk_keyseed_value(int kyber_k, const uint8_t *sk, const uint8_t *context, const uint8_t *salt, uint8_t seed[32])
{
    Params P;
    if (!make_params(kyber_k, P) || !sk || !seed) return -1;
    return guard(static_cast<const kosk_ctx *>(nullptr), __func__, [&]() -> int {
    keyseed_value(P, sk, context, salt, seed);
    return 0;
    GUARD_END
}
int kosk_fs_alpha_bound(int kyber_k, const uint8_t *tcomm_all, const uint8_t bind[32], uint16_t *alpha)
{
    Params P;
    if (!make_params(kyber_k, P) || !tcomm_all || !bind || !alpha) return -1;
    return guard(static_cast<const kosk_ctx *>(nullptr), __func__, [&]() -> int {
    fs_alpha(P, tcomm_all, alpha, bind);
    return 0;
    GUARD_END
}
int kosk_fs_opened_bound(const uint8_t *digests_all, const uint8_t bind[32], uint16_t *I, uint16_t *rest)
{
    if (!digests_all || !bind || !I || !rest) return -1;
    return guard(static_cast<const kosk_ctx *>(nullptr), __func__, [&]() -> int {
    fs_opened(digests_all, I, rest, bind);
    return 0;
    GUARD_END
}

void kosk_host_sha3_256(uint8_t out[32], const uint8_t *in, size_t inlen) { sha3_256(out, in, inlen); }
void kosk_host_shake256(uint8_t *out, size_t outlen, const uint8_t *in, size_t inlen) { shake256(out, outlen, in, inlen); }

int kosk_host_sha3_256_multi(uint8_t *out, const uint8_t *in, size_t in_stride, size_t inlen, int count, int nthreads)
{
    // same code path as the batched Fiat-Shamir rounds: SIMD groups spread over the pool
    if (!out || !in || count < 0) return -1;
    return guard(static_cast<const kosk_ctx *>(nullptr), __func__, [&]() -> int {
    std::vector<const uint8_t *> ptr(count);
    for (int i = 0; i < count; i++) ptr[i] = in + (size_t)i * in_stride;
    const int w = sha3_multi_width();
    if (nthreads <= 1) { sha3_256_multi(out, ptr.data(), inlen, count); return w; }
    const int groups = (count + w - 1) / w;
    parallel_for(groups, nthreads, [&](int g) {
        const int lo = g * w, n = (count - lo) < w ? (count - lo) : w;
        sha3_256_multi(out + 32 * (size_t)lo, ptr.data() + lo, inlen, n);
    });
    return w;
    GUARD_END
}

int kosk_lagrange_table(int which, uint16_t *out)
{
    if (!out) return -1;
    return guard(static_cast<const kosk_ctx *>(nullptr), __func__, [&]() -> int {
    if (which == 0) {
        for (int x = 0; x < NPARTY - NOPEN - 1; x++) lagrange_row(out + (size_t)x * XLEN, XLEN, 0, XLEN + x);
    } else if (which == 1) {
        for (int i = 0; i < NSEC; i++) lagrange_row(out + (size_t)i * XLEN, XLEN, NSEC, i);
    } else if (which == 2) {
        for (int i = 0; i < NSEC; i++) lagrange_row(out + (size_t)i * (DEG2 + 1), DEG2 + 1, NSEC, i);
    } else {
        return -1;
    }
    return 0;
    GUARD_END
}

} // extern "C"
