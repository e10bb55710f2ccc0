/*
 * kosk_mi355x.h -- C ABI of the MI355X-native KOSK prover/verifier.
 *
 * Drop-in boundary for the reference's hot path (ZGC-SP/mpcith_kyber_kosk).
 * Every entry point names the reference interface it replaces (file:line
 * relative to the reference root).  Plain pointers and sizes only; the library
 * owns all device memory.  All functions return 0 on success and a negative
 * value on error (kosk_last_error() gives the text) unless stated otherwise.
 * There is no CPU fallback: kosk_create() fails when no HIP device is present.
 *
 * Parameter sets: kyber_k in {2,3,4} is a run-time argument here; in the
 * reference it is the compile-time macro KYBER_K (params.hpp:8-10).
 */
#ifndef KOSK_MI355X_H
#define KOSK_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct kosk_ctx kosk_ctx;

/* Replaces the link-time symbol randombytes() (kyber/randombytes.h:7).  The
 * library calls it in exactly the reference's order and lengths for each
 * proof: 64, M x 32, then 302-byte draws. */
typedef void (*kosk_randombytes_fn)(void *user, uint8_t *out, size_t len);

/* sizes: KYBER_PUBLICKEYBYTES / KYBER_SECRETKEYBYTES (kyber/params.h:49-52),
 * MPCITH_PROOF_SIZE (mlwe_prover.hpp:30), randomness per verifiable keygen */
size_t kosk_pk_bytes(int kyber_k);
size_t kosk_sk_bytes(int kyber_k);
size_t kosk_proof_bytes(int kyber_k);
size_t kosk_tape_bytes(int kyber_k);
/* byte offset / size of field `idx` (0..23, declaration order of mpcith_proof,
 * mlwe_prover.hpp:57-75) inside the proof image; returns 0 on success */
int kosk_proof_field(int kyber_k, int idx, size_t *offset, size_t *size);

/* ---- Seeded proving (no reference counterpart: the reference draws every tape byte with randombytes, kosk.cpp:12,
 * mlwe_prover.cpp:9, ss.cpp:5).  Format kosk-seedtape-v1: with T = kosk_tape_bytes(kyber_k),
 *   block_j = SHAKE256(seed[32] || "kosk-seedtape-v1" || LE32(kyber_k) || LE32(j))[0 : 136],  j = 0 .. ceil(T / 136) - 1
 *   tape    = (block_0 || block_1 || ...)[0 : T]
 * (counter mode: every block is one independent Keccak-f[1600]).  A seeded call returns byte for byte what the explicit-tape call
 * returns on that tape.  A seed determines the key seed and all masking randomness of its proof: it is as secret as the secret key
 * and must be used once. */
#define KOSK_SEED_BYTES 32
/* host, no handle: the tape of one seed (kosk_tape_bytes(kyber_k) bytes); -1 for kyber_k outside 2..4 or a null pointer */
int kosk_tape_from_seed(int kyber_k, const uint8_t seed[KOSK_SEED_BYTES], uint8_t *tape);

int kosk_create(kosk_ctx **ctx, int device, int kyber_k, int max_batch);

/* ---- Per-handle options (round 6).  The reference has no run-time configuration at all (kosk.hpp:18-24 takes pointers, nothing
 * else); what a HOST must decide per handle -- how its calls are batched, what the verifier accepts, where the Fiat-Shamir rounds
 * run, how its threads wait -- is this struct, not the process environment.  kosk_options_init() fills in "not given" for every
 * field (the library's defaults apply); kosk_create_ex() with opt == NULL is kosk_create().  The environment variables of the same
 * names that earlier rounds read at kosk_create() (KOSK_STREAMS, KOSK_COMBINE, KOSK_FS_DEVICE, ...) are no longer read by either call;
 * only debug knobs remain in the environment. */
enum { KOSK_FS_HOST = 0, KOSK_FS_DEVICE = 1 };
typedef struct kosk_options {
    uint32_t size;              /* sizeof(kosk_options) as the caller compiled it (set by kosk_options_init) */
    int32_t streams;            /* sub-batches of a batch call in flight on separate HIP streams, 1..8; 0: not given = 1 */
    int32_t combine;            /* handles per cohort whose resident calls are merged, 2..16 (call combining, see below); 0: not given, 1: off */
    int32_t combine_wait_us;    /* longest wait of a call for the cohort's other members (default 5000); < 0: not given */
    int32_t combine_idle_us;    /* a member that left a call longer ago than this is not waited for (default 1000); < 0: not given */
    int32_t combine_prewake_us; /* how long the sleeping callers of a merged run may spin for its return (default 400); < 0: not given */
    int32_t strict_encoding;    /* verifier: 1 (DEFAULT) a u16 element >= q in any record the reference reads marks the proof malformed;
                                 * 0 the reference-following mode (accepts what the reference accepts: non-canonical encodings are then
                                 * malleable); < 0: not given */
    int32_t fs_mode;            /* KOSK_FS_HOST: the Fiat-Shamir hashes run on the host's cores (digest tables cross PCIe, four host
                                 * round trips per prove + verify); KOSK_FS_DEVICE: one wave per proof hashes the tables in HBM, alpha /
                                 * I / the verifier's I' == I stay on the device, the resident calls have no host round trip; < 0: not given */
    int32_t host_threads;       /* Fiat-Shamir / key-assembly workers of this handle; 0: not given */
    int32_t blocking_sync;      /* 1: the handle's host waits sleep on events instead of spinning (few cores per GPU); < 0: not given */
    int32_t hooks_unmerged;     /* 1: while this handle has a round hook (kosk_set_round_hook) its calls never join a merged run: the hook
                                 * then always fires on the handle's OWN calling thread (thread-local state, blocking hooks); 0 / < 0: merged */
    int32_t reserved[6];        /* zero */
} kosk_options;
void kosk_options_init(kosk_options *opt);
int kosk_create_ex(kosk_ctx **ctx, int device, int kyber_k, int max_batch, const kosk_options *opt);
void kosk_destroy(kosk_ctx *ctx);
const char *kosk_last_error(const kosk_ctx *ctx); /* ctx may be NULL: error of the last failed kosk_create */
int kosk_set_randombytes(kosk_ctx *ctx, kosk_randombytes_fn fn, void *user); /* NULL: OS entropy */
/* What a call with `tapes` == NULL draws through the randombytes callback / OS entropy (a setter like kosk_set_randombytes, applied to
 * every sub-context of the handle; not a field of kosk_options).  KOSK_ENTROPY_TAPE (the default of every handle): the reference's
 * sequence of 64, M x 32 and 302-byte calls per proof, a whole tape.  KOSK_ENTROPY_SEED: ONE call of KOSK_SEED_BYTES per proof, in
 * proof order; the call then behaves as its *_seeded form below with seeds == NULL.  Any other mode: -1, nothing changed. */
enum { KOSK_ENTROPY_TAPE = 0, KOSK_ENTROPY_SEED = 1 };
int kosk_set_entropy(kosk_ctx *ctx, int mode);

/* ---- Erasing secrets.  The handle keeps an inventory of every buffer it owns, in HBM and in page-locked host
 * memory, and of which of them can hold secret-derived bytes: the row matrix, tapes and seeds, s / e and their NTTs, the NTT(s) bytes
 * and sha3_512 output of the key records, the sk copies and salts of the calls on existing keys, the offline bank, and the KEM workspace except its
 * public keys, ciphertexts, A, H(pk) and flags.
 * kosk_wipe_secrets zeroes all of those now (one launch of k_wipe for the HBM regions, the host for the page-locked staging) and returns
 * when that is done.  It must not be called while another thread is inside a call on the handle.  Afterwards the handle is as usable
 * as before, and its PUBLIC resident state is untouched: kosk_fetch_proofs*, kosk_resident_proofs, kosk_resident_digests,
 * kosk_verify_resident_pk(pk == NULL), kosk_kem_enc_verified and kosk_verify_fail_masks behave exactly as without the wipe.  Staged
 * prover inputs are gone: kosk_prove_resident returns -1 ("staged inputs were wiped") until a staging call has run again.  Memory of
 * the caller -- its buffers, device tapes read in place -- is never touched.
 * kosk_set_wipe(KOSK_WIPE_CALL): every entry point that brings secrets onto the handle ends with that wipe, on success and on every
 * error return: the key generations in every form, kosk_prove_resident, kosk_prove_prepared, kosk_prepare_*, kosk_kem_enc_batch /
 * _dec_batch / _enc_verified / _keypair_batch, kosk_kem_check_sk, kosk_keyseed_device, kosk_tape_expand_device and kosk_prove_keys_*;
 * kosk_bank_fill, kosk_prove_keys_banked_batch and kosk_verifiable_keygen_banked_batch (everything but the unconsumed entries of the
 * offline bank, a long-lived secret like the resident key; only kosk_wipe_secrets, kosk_bank_reserve(0) and kosk_destroy erase those);
 * kosk_kem_enc_key / _dec_key (their per-call scratch; the resident key of kosk_kem_key_set is a long-lived secret and stays);
 * chunked calls and streams > 1 wipe every sub-context.  Not the staging calls (kosk_stage_prover_inputs*, kosk_stage_prover_keys*,
 * kosk_stage_prover_keys_banked, kosk_witness_from_sk): their secrets are the input of the kosk_prove_resident that follows, which wipes when it ends.  A member of
 * a cohort (combine >= 2) in this mode keeps its calls out of merged runs, exactly as an armed handle does, and wipes its own block of
 * the shared workspace.  One difference: kosk_combine_stats counts an armed member's solo runs (calls == members) and leaves the solo
 * runs of a member in this mode out (0, 0).  KOSK_WIPE_OFF is the default; any other mode: -1, nothing changed.  With the mode off every call returns
 * the bytes it returned before these calls existed.
 * kosk_destroy always wipes before it frees; the last member of a cohort to be destroyed wipes the whole shared workspace.
 * kosk_secret_scan is the audit: *hits = the number of byte positions at which needle[0, len), 16 <= len <= 64, occurs in ANY buffer
 * of the inventory, secret or public, HBM (k_scan) and page-locked host memory -- so that a buffer filed under the wrong heading
 * shows.  A diagnostic: unmerged, synchronised, not constant-time in the needle; its own device copy of the needle is cleared before
 * it returns.  -1 for a NULL argument or len out of range. */
enum { KOSK_WIPE_OFF = 0, KOSK_WIPE_CALL = 1 };
int kosk_wipe_secrets(kosk_ctx *ctx);
int kosk_set_wipe(kosk_ctx *ctx, int mode);
int kosk_secret_scan(kosk_ctx *ctx, const uint8_t *needle, size_t len, long *hits);
/* kernel level (tests): k_wipe on the CALLER's device memory, region i = [d_ptrs[i], d_ptrs[i] + bytes[i]), any alignment, any length
 * (0: skipped), any number of regions; nothing outside the regions is written.  Runs on the handle's own stream, synchronised on return. */
int kosk_wipe_device(kosk_ctx *ctx, int nregions, void *const *d_ptrs, const size_t *bytes);
/* UNSTABLE, not part of the supported interface: a diagnostic for tools/wipe_rate.py that may change or go without notice, and that WIPES
 * THE HANDLE as a side effect (staged inputs included).  It wipes the handle (streams = 1, or sub-batch 0 of it) and then times `reps` launches of k_wipe over its
 * secret HBM regions and `reps` rounds of the runtime's own fills of the same regions (one hipMemsetAsync per region), each between
 * two events on the handle's stream.  *bytes / *regions (may be NULL): what one wipe clears in HBM. */
int kosk_wipe_timing(kosk_ctx *ctx, int reps, double *wipe_ms, double *memset_ms, size_t *bytes, int *regions);

/* void kyber_verifiable_keygen(kyber_keypair *keypair, uint8_t *pi)   kosk.hpp:20-21, kosk.cpp:72-86
 * n independent instances; pk/sk/pi are n consecutive records of kosk_*_bytes().
 * `tapes` == NULL draws randomness through the randombytes callback; otherwise
 * proof b consumes tapes[b*tape_stride ..] (kosk_tape_bytes() bytes each).
 * Error containment (all entry points): no C++ exception and no abort leaves the library -- a failed allocation, thread or
 * HIP call is rc -1 + kosk_last_error(); the only abort is the reference's own, an OS entropy failure
 * (kyber/randombytes.c:49-52).  A batch call creates no threads (kosk_create made them).
 * HIP error state: the library's launchers read hipGetLastError(), so every entry point first RESETS the calling thread's HIP
 * last-error state; an application that launches kernels of its own must check them before it calls in here.
 * The library never page-locks caller memory (KOSK_REGISTER=2 of rounds 2-4, which did so for the duration of a multi-chunk call,
 * was removed in round 5: the two process aborts on record both happened inside calls that had just page-locked Python heap
 * memory and were never explained; the value is now read as 1).
 * gen_matrix's rejection sampling (indcpa.c:124-145) loops without a bound in the reference; on the host this library does the
 * same, on the GPU it squeezes at most 32 SHAKE128 blocks per matrix entry (three suffice with probability 1 - 2^-40) and a
 * call that ever reached that limit returns -1 ("block limit") without results -- for key generation and for the verifier's
 * decoding of a public key alike. */
int kosk_verifiable_keygen_batch(kosk_ctx *ctx, int n, const uint8_t *tapes, size_t tape_stride,
                                 uint8_t *pk, uint8_t *sk, uint8_t *pi);

/* The seeded forms of the four calls that take tapes at the reference's first level: proof b uses the tape of the seed at
 * seeds + b * seed_stride (seed_stride >= KOSK_SEED_BYTES; host or DEVICE memory).  seeds == NULL: the library draws one
 * KOSK_SEED_BYTES call per proof, in proof order, through the randombytes callback / OS entropy.  The seeds (32 bytes per proof) are
 * the only randomness that crosses PCIe; the tapes are expanded in HBM (k_tape_expand) on the handle's stream.  Chunking, streams and
 * call combining as for the tape forms: a merged run of a cohort may mix seeded callers with callers that bring device or host tapes. */
int kosk_verifiable_keygen_seeded_batch(kosk_ctx *ctx, int n, const uint8_t *seeds, size_t seed_stride, uint8_t *pk, uint8_t *sk, uint8_t *pi);
int kosk_verifiable_keygen_seeded_batch_compact(kosk_ctx *ctx, int n, const uint8_t *seeds, size_t seed_stride, uint8_t *pk, uint8_t *sk,
                                                uint8_t *out);
int kosk_verifiable_keygen_seeded_resident(kosk_ctx *ctx, int n, const uint8_t *seeds, size_t seed_stride, uint8_t *pk, uint8_t *sk);
int kosk_stage_prover_inputs_seeded(kosk_ctx *ctx, int n, const uint8_t *seeds, size_t seed_stride, uint8_t *pk, uint8_t *sk);

/* Page-locked host memory for the proof buffers of the two host-buffer calls (no reference counterpart: the reference's
 * caller owns plain arrays, main.cpp:71).  Proof images in such a buffer (or in any memory the caller page-locked itself with
 * hipHostMalloc / hipHostRegister) cross PCIe straight from / to it: no staging copy on the host and no per-call locking.
 * Plain (pageable) buffers keep working through the library's pinned staging buffers.  NULL on failure. */
void *kosk_host_alloc(size_t bytes);
void kosk_host_free(void *p);

/* bool kyber_kosk_verify(const uint8_t *pi, const uint8_t *pk)       kosk.hpp:23-24, kosk.cpp:88-117
 * ok[b] = 1 accept / 0 reject.  The reference prints a diagnostic and returns
 * false (mlwe_verifier.cpp:120 etc.); here kosk_verify_fail_masks() reports
 * which checks failed (bit i = check i of DESIGN.md's verifier table). */
int kosk_verify_batch(kosk_ctx *ctx, int n, const uint8_t *pi, const uint8_t *pk, uint8_t *ok);
int kosk_verify_fail_masks(const kosk_ctx *ctx, uint32_t *masks, int n); /* n <= proofs of the last completed verify call */

/* ---- Second-level entry points of the reference (mlwe_prover.hpp:77-99, mlwe_verifier.hpp:14-15; used directly by
 * main.cpp:21-47) on n instances at a time.  The buffers are arrays of the reference's structs for this kyber_k, byte for
 * byte (little-endian, no padding):
 *   share_vec          { uint64 len = 1454; u16 share_x[1454] (= 256 + party); u16 share_y[1454]; }      ss.hpp:33-37
 *   mpcith_randomness  { u16 f[M][256]; u16 NTT_f[M][256]; share_vec f_shares[M]; share_vec NTT_f_shares[M]; }   M = 71 + 2K
 *   mpcith_range_proof { share_vec s_eta_shares[K][2 eta1 + 1]; share_vec e_eta_shares[K][2 eta1 + 1]; }
 *   mlwe_inst          { i16 A[K][K][256] (NTT domain); i16 t[K][256]; i16 s[K][256]; i16 e[K][256]; }   = kosk_keygen's outputs
 * Randomness: `tapes` = per instance exactly the bytes the reference would draw in that call, in its order
 * (prepare_randomness: M x 32 then 2M x 302; prepare_range_proof: 2K(2 eta1 + 1) x 302; prove: (3K + 4K eta1) x 302),
 * tape_stride apart; NULL = the randombytes callback / OS entropy with the reference's call sequence. */
size_t kosk_randomness_bytes(int kyber_k);  /* sizeof(mpcith_randomness)  */
size_t kosk_range_proof_bytes(int kyber_k); /* sizeof(mpcith_range_proof) */
size_t kosk_mlwe_inst_bytes(int kyber_k);   /* sizeof(mlwe_inst)          */
/* prepare_randomness, mlwe_prover.cpp:4-39 */
int kosk_prepare_randomness(kosk_ctx *ctx, int n, const uint8_t *tapes, size_t tape_stride, uint8_t *rand_out);
/* prepare_range_proof, mlwe_prover.cpp:41-59 */
int kosk_prepare_range_proof(kosk_ctx *ctx, int n, const uint8_t *tapes, size_t tape_stride, uint8_t *range_out);
/* prove + encode_mpcith_proof, mlwe_prover.cpp:81-543: pi receives n proof images.  What the call reads, as the reference's prove():
 *   mpcith_randomness   share_y of f_shares[] and NTT_f_shares[] only.  f and NTT_f are NOT read (prove() computes everything from the
 *                       shares; the opened s + r is recon_secrets_ddeg of parties 0..406, and so it is here: the packed secrets of the 2M
 *                       rows are reconstructed on the GPU from those parties).  A caller may bank the shares and drop, zero or overwrite
 *                       the two secret members; rows that lie on no degree-406 polynomial give the reference's bytes too.
 *   mpcith_range_proof  share_y of every sharing.  PRECONDITION: s_eta_shares[i][j] and e_eta_shares[i][j] are valid sharings (degree
 *                       406) of the constant j - eta1 at all 256 packed positions, as prepare_range_proof makes them, with any 151 free
 *                       points; the struct has no secrets member to check them against, and other contents are not supported.
 *   mlwe_inst           A (any int16 representative mod q), s and e.  t is not read.  s and e must lie in [-(q - 1), q - 1] = [-3328,
 *                       3328]: outside it encode_to_gf3329 is not canonical and nothing downstream is defined; the call refuses (-1).
 *   share_vec           len and share_x are implied (1454, 256 + party) and ignored.
 * Every share_y must be canonical (< q = 3329): the call returns -1 with a text (kosk_last_error) otherwise. */
int kosk_prove_prepared(kosk_ctx *ctx, int n, const uint8_t *inst, const uint8_t *rand_in, const uint8_t *range_in,
                        const uint8_t *tapes, size_t tape_stride, uint8_t *pi);
/* decode_mpcith_proof + verify, mlwe_verifier.cpp:4-686, with A and t from the instance (s, e are not read).  A: any int16 representative
 * mod q.  t: compared as the reference compares it, encode_to_gf3329(t) (q + t for t < 0, else t; nothing reduced) against the canonical
 * t of the proof (:358), so a coefficient outside [-q, q - 1] fails check 5 whatever its residue */
int kosk_verify_inst(kosk_ctx *ctx, int n, const uint8_t *pi, const uint8_t *inst, uint8_t *ok);

/* Device-resident split of the two calls above, for callers that keep inputs
 * and proofs in HBM (and for bench.py: the timed region is *_resident only). */
int kosk_stage_prover_inputs(kosk_ctx *ctx, int n, const uint8_t *tapes, size_t tape_stride, uint8_t *pk, uint8_t *sk);
int kosk_prove_resident(kosk_ctx *ctx, int n);
int kosk_fetch_proofs(kosk_ctx *ctx, int n, uint8_t *pi);
int kosk_stage_verifier_inputs(kosk_ctx *ctx, int n, const uint8_t *pi, const uint8_t *pk);
int kosk_verify_resident(kosk_ctx *ctx, int n, uint8_t *ok);
/* The two reference calls as ONE resident call each (what bench.py times):
 * kyber_verifiable_keygen (kosk.cpp:72-86) -- key generation (kosk.cpp:4-70) runs on the device at the head of the
 * prover's first segment, pk / sk are written to the HOST buffers, the proofs stay in HBM.  `tapes` may be host or DEVICE
 * memory (a device buffer whose base and tape_stride are multiples of 8 is read in place) or NULL (randombytes callback).
 * kyber_kosk_verify (kosk.cpp:88-117) on the resident proofs -- polyvec_frombytes(t) + gen_matrix (kosk.cpp:94-99) run at
 * the head of the verifier's first segment from `pk` (host or device memory), or, with pk == NULL, from the pk bytes the
 * key generation (or a verifier staging call) of at least n proofs left in HBM on this handle -- an error otherwise.
 * A DEVICE tape buffer that is read in place must stay valid and unmodified until the prove call that consumes it has
 * returned (kosk_verifiable_keygen_resident itself, or kosk_prove_resident after kosk_stage_prover_inputs). */
int kosk_verifiable_keygen_resident(kosk_ctx *ctx, int n, const uint8_t *tapes, size_t tape_stride, uint8_t *pk, uint8_t *sk);
int kosk_verify_resident_pk(kosk_ctx *ctx, int n, const uint8_t *pk, uint8_t *ok);
/* ---- Compact wire format (no reference counterpart: the reference ships the raw image of
 * mpcith_proof, mlwe_prover.cpp:540-543).  Same 24 fields in the same order, every u16 field packed two values into
 * three bytes (12 bits each, the bit order of Kyber's poly_tobytes, kyber/poly.c:128-147), the two digest fields raw,
 * every field on a 16-byte boundary: 664 340 / 680 980 / 744 148 -> 78 % of that.  Lossless for images whose u16
 * values are below 4096 (compression fails otherwise).  The resident variants pack / unpack on the GPU so that PCIe
 * carries the compact bytes. */
size_t kosk_compact_proof_bytes(int kyber_k);
int kosk_proof_compress(int kyber_k, const uint8_t *pi, uint8_t *out);   /* host codec; -1 if a value >= 4096 */
int kosk_proof_decompress(int kyber_k, const uint8_t *in, uint8_t *pi);
/* kosk_verifiable_keygen_batch / kosk_verify_batch with the proofs in the compact format: n records of
 * kosk_compact_proof_bytes(); any n (chunked like the image calls), host or page-locked host buffers */
int kosk_verifiable_keygen_batch_compact(kosk_ctx *ctx, int n, const uint8_t *tapes, size_t tape_stride,
                                         uint8_t *pk, uint8_t *sk, uint8_t *out);
int kosk_verify_batch_compact(kosk_ctx *ctx, int n, const uint8_t *in, const uint8_t *pk, uint8_t *ok);
int kosk_fetch_proofs_compact(kosk_ctx *ctx, int n, uint8_t *out);        /* like kosk_fetch_proofs */
int kosk_stage_verifier_inputs_compact(kosk_ctx *ctx, int n, const uint8_t *in, const uint8_t *pk); /* like kosk_stage_verifier_inputs */

/* ---- Dense wire format kosk-dense-v1 (INTEGRATION.md 11 is the normative text; no reference counterpart).  The compact format's
 * layout -- the 24 fields in order, each on a 16-byte boundary, Tcomm and comm raw, every u16 field 12 bits per value in
 * poly_tobytes bit order, an odd number of stored values packed with one trailing zero value -- but fields 2, 3, 8, 13, 14, 15, 16
 * (beta, gamma, t, s+r, e+r, s_eta, e_eta shares of the 1304 unopened parties in ascending order) store rows 0..406 only: their rows
 * hold evaluations of polynomials of degree <= 406 at the points 256 + party, so rows 407..1303 are the Lagrange interpolation of
 * rows 0..406 (mod q) through the nodes 256 + rest[j], rest = ascending complement of I.  285 184 / 290 912 / 320 800 bytes for
 * kyber_k 2 / 3 / 4: 43 % of the image.  The image and the compact format are unchanged; a dense record verifies exactly as the
 * image it unpacks to (same bit, same fail mask, either strict_encoding mode, armed or not).
 * Host codec (no device): kosk_proof_dense_pack returns 0, -1 for a stored value >= 4096, -2 for a malformed I (an entry >= 1454 or
 * repeated) or a row >= 407 of a listed field that is not the refill -- it succeeds iff unpack(pack(image)) == image.
 * kosk_proof_dense_unpack returns 0, or 1 for a malformed I: rows 407..1303 of the listed fields are then zero (the verifier rejects
 * every image with such an I); -1 for bad arguments.  Refilled values are canonical; stored values up to 4095 survive unreduced. */
size_t kosk_dense_proof_bytes(int kyber_k);
int kosk_proof_dense_pack(int kyber_k, const uint8_t *pi, uint8_t *out);
int kosk_proof_dense_unpack(int kyber_k, const uint8_t *in, uint8_t *pi);
/* The compact calls' counterparts: n records of kosk_dense_proof_bytes(), packed on the GPU in front of the D2H copy, unpacked and
 * refilled on the GPU behind the H2D copy.  Chunking, streams, page-locked and pageable buffers, armed handles and "never merged" as
 * for the compact calls.  Packing does not check that the resident images are representable: what this library's prover leaves in
 * HBM is (the zero-witness proof at an ok[b] = 0 position of kosk_stage_prover_keys* included); foreign images go through
 * kosk_transcode_batch below, which checks. */
int kosk_verifiable_keygen_batch_dense(kosk_ctx *ctx, int n, const uint8_t *tapes, size_t tape_stride, uint8_t *pk, uint8_t *sk, uint8_t *out);
int kosk_verifiable_keygen_seeded_batch_dense(kosk_ctx *ctx, int n, const uint8_t *seeds, size_t seed_stride, uint8_t *pk, uint8_t *sk,
                                              uint8_t *out);
int kosk_verify_batch_dense(kosk_ctx *ctx, int n, const uint8_t *in, const uint8_t *pk, uint8_t *ok);
int kosk_fetch_proofs_dense(kosk_ctx *ctx, int n, uint8_t *out);        /* like kosk_fetch_proofs */
int kosk_stage_verifier_inputs_dense(kosk_ctx *ctx, int n, const uint8_t *in, const uint8_t *pk); /* like kosk_stage_verifier_inputs */
/* kernel level: the refill alone on n >= 1 images in HBM, in place (image b at d_images + b * image_stride; both 16-byte aligned,
 * image_stride >= kosk_proof_bytes).  d_status (device memory, n x uint32): 0, or 1 for a malformed I, in which case image b is not
 * written.  Nothing outside rows 407..1303 of the seven listed fields is changed.  Runs on the handle's own stream, synchronised on return. */
int kosk_dense_fill_device(kosk_ctx *ctx, int n, uint8_t *d_images, size_t image_stride, uint32_t *d_status);

/* ---- Transcoding between the three wire formats on the GPU: image <-> compact <-> dense, n >= 1 records per call
 * (chunked by max_batch), for a party that stores, forwards or translates proofs and holds no keys.  `in` is n consecutive records of
 * kosk_format_bytes(k, from), `out` n consecutive records of kosk_format_bytes(k, to); each of the two is host memory (pageable or
 * page-locked) or device memory of ANY alignment, told apart per pointer as the KEM calls do (the library copies into its own aligned
 * workspace); they must not overlap.  `status` is host memory, n entries.  from == to is refused.
 * The contract is the composition of the host codecs, per record b:
 *   1. decode `from` into an image: compact kosk_proof_decompress; dense kosk_proof_dense_unpack (result 1: a malformed I, rows 407..1303
 *      of the listed fields left zero); an image decodes to itself;
 *   2. encode that image into `to`: compact kosk_proof_compress (-1: a value >= 4096); dense kosk_proof_dense_pack (-1 or -2, with the host
 *      code's precedence: -1 concerns STORED values only and wins over -2; a value >= 4096 in a dropped row is -2, not -1); an image
 *      encodes to itself;
 *   3. status[b] = the encoder's result if it is nonzero, otherwise the decoder's.
 * For status[b] >= 0 (status 1 included) `out` record b is byte for byte what the host codecs produce; for status[b] < 0 it is all zero
 * (the host codecs leave it unspecified; this call defines it).  Other positions are unaffected.
 * Returns 0 when it ran, whatever the statuses are; -1 with a kosk_last_error text, nothing started, for NULL arguments, n < 1, a bad
 * format, from == to or overlapping buffers.
 * The call touches none of the prover's, verifier's or KEM's resident state: kosk_fetch_proofs*, kosk_resident_proofs,
 * kosk_verify_resident_pk(pk == NULL) and kosk_kem_enc_verified behave after it as before it.  Its workspace (max_batch images, the
 * records of both sides, two status words per record) is allocated at the handle's first such call and filed in the buffer inventory as
 * PUBLIC buffers: kosk_secret_scan sees them, kosk_wipe_secrets leaves them, kosk_destroy frees them.  It brings no secret onto the
 * handle and is not one of the entry points that wipe under KOSK_WIPE_CALL.  It runs unmerged on a cohort member, and with streams > 1
 * on sub-batch 0's stream. */
enum { KOSK_FMT_IMAGE = 0, KOSK_FMT_COMPACT = 1, KOSK_FMT_DENSE = 2 };
size_t kosk_format_bytes(int kyber_k, int fmt);      /* kosk_proof_bytes / kosk_compact_proof_bytes / kosk_dense_proof_bytes / (fmt 4, below) kosk_dense2_proof_bytes; 0 for a bad k or fmt */
int kosk_transcode_batch(kosk_ctx *ctx, int n, int from, const uint8_t *in, int to, uint8_t *out, int32_t *status);
/* kernel level: the codeword check alone on n >= 1 images in the caller's HBM (alignment rules of kosk_dense_fill_device; -1 and a text
 * otherwise).  Strictly read-only on the images.  d_status[b] (device memory, n x uint32): 0; 1 a malformed I; 2 some u16 in rows
 * 407..1303 of a listed field differs from the refill of rows 0..406 -- the refill is canonical, so a congruent value v + q in a dropped
 * row is a difference.  It says nothing about values >= 4096 in kept rows (the pack kernel's overflow word does).  Runs on the handle's
 * own stream, synchronised on return. */
int kosk_dense_check_device(kosk_ctx *ctx, int n, const uint8_t *d_images, size_t image_stride, uint32_t *d_status);

/* ---- Dense wire format kosk-dense-v2 (INTEGRATION.md 11.2 is the normative text).  Everything of kosk-dense-v1 holds except the stored
 * rows of four fields whose sharing polynomials have PUBLIC values at the 256 packed positions x = 0..255:
 *   fields 15, 16 (s_eta, e_eta shares) store rows 0..150: column c shares the constant kappa_c = (c mod (2 eta1 + 1)) - eta1 mod q at
 *     all 256 positions (the verifier's fail bit 7 insists on it), so a polynomial of degree <= 406 has 151 free values;
 *   fields 21, 22 (u_s, u_e shares of degree <= 812) store rows 0..556: u is zero at all 256 positions (fail bit 9).
 * With Z(x) = prod_{a < 256} (x - a) every such column is p = kappa + Z v, and the dropped rows are rebuilt from v's interpolation
 * through the nodes 256 + rest[j], j < 151 / 557.  Fields 2, 3, 8, 13, 14 stay at rows 0..406 with v1's refill.
 * 247 552 / 252 512 / 269 600 bytes for kyber_k 2 / 3 / 4: 37 % of the image.  A v2 record verifies exactly as the image it unpacks to;
 * every image the verifier accepts is representable; an image whose eta rows lie on a degree-406 polynomial with OTHER values at the
 * packed positions packs to v1 and gives -2 here.  v1 records stay valid and byte-identical.
 * Host codec: the return codes of the v1 codec, on v2's stored and dropped rows (pack 0 / -1 a stored value >= 4096, it wins / -2;
 * unpack 0 / 1 a malformed I, rows 407.. of the five v1 fields, 151.. of fields 15 / 16 and 557.. of fields 21 / 22 then zero). */
enum { KOSK_FMT_DENSE2 = 4 }; /* a separate enum: 0..2 above are pinned.  3 is not a format and will not become one */
size_t kosk_dense2_proof_bytes(int kyber_k); /* = kosk_format_bytes(kyber_k, KOSK_FMT_DENSE2) */
int kosk_proof_dense2_pack(int kyber_k, const uint8_t *pi, uint8_t *out);
int kosk_proof_dense2_unpack(int kyber_k, const uint8_t *in, uint8_t *pi);
/* kernel level, the contracts of kosk_dense_fill_device / kosk_dense_check_device on v2's dropped rows: status 0 / 1 / 2, nothing outside
 * the refilled rows is written, the check is strictly read-only. */
int kosk_dense2_fill_device(kosk_ctx *ctx, int n, uint8_t *d_images, size_t image_stride, uint32_t *d_status);
int kosk_dense2_check_device(kosk_ctx *ctx, int n, const uint8_t *d_images, size_t image_stride, uint32_t *d_status);
/* kosk_transcode_batch takes KOSK_FMT_DENSE2 on either side (12 ordered pairs; the composition rule above with the v2 codec).
 * The five host-buffer calls with the packed format as an argument, so that a further format needs no further names: fmt =
 * KOSK_FMT_COMPACT / KOSK_FMT_DENSE run the bodies of the _compact / _dense calls (same bytes, return codes, argument-check order,
 * counters and resident-state effects); KOSK_FMT_DENSE2 behaves the same way in the new format (chunked by max_batch, streams, pageable
 * and page-locked buffers, armed handles, never merged; a verifier staging call counts as "replaced the resident keys" for
 * kosk_kem_enc_verified).  Any other fmt, the image included, is refused with a text that names the format. */
int kosk_verifiable_keygen_batch_fmt(kosk_ctx *ctx, int fmt, int n, const uint8_t *tapes, size_t tape_stride, uint8_t *pk, uint8_t *sk, uint8_t *out);
int kosk_verifiable_keygen_seeded_batch_fmt(kosk_ctx *ctx, int fmt, int n, const uint8_t *seeds, size_t seed_stride, uint8_t *pk, uint8_t *sk,
                                            uint8_t *out);
int kosk_verify_batch_fmt(kosk_ctx *ctx, int fmt, int n, const uint8_t *in, const uint8_t *pk, uint8_t *ok);
int kosk_fetch_proofs_fmt(kosk_ctx *ctx, int fmt, int n, uint8_t *out);
int kosk_stage_verifier_inputs_fmt(kosk_ctx *ctx, int fmt, int n, const uint8_t *in, const uint8_t *pk);

/* ---- Kyber KEM on the keys this library makes and vouches for: crypto_kem_enc_derand / crypto_kem_enc / crypto_kem_dec
 * (kyber/kem.c:76-96, :113-121, :140-169; indcpa_enc / indcpa_dec, kyber/indcpa.c:264-336), bit-exact, for kyber_k 2 / 3 / 4, n items
 * per call.  Records are consecutive: kosk_pk_bytes, kosk_sk_bytes (s || pk || H(pk) || z, what kosk_verifiable_keygen_* returns),
 * kosk_ct_bytes, KOSK_SS_BYTES.  Every buffer may be host or device memory (told apart like the seeds of the seeded calls).  n is any
 * positive number: the calls work through launch groups of 16384 items.  The KEM workspace (about 13 KB per item of the largest launch group
 * the handle has seen, for kyber_k = 4) is allocated at a handle's first KEM call; a handle that never makes one takes no HBM for it.
 * coins: n x 32 bytes, the m of crypto_kem_enc_derand; NULL: one 32-byte draw per item, in item order, on the caller's thread, through
 * the randombytes callback / OS entropy (kem.c:117-118).
 * Encoding: like the reference's polyvec_frombytes these calls take any 12-bit coefficient in a pk or sk and compute with it mod q
 * (the ciphertext then differs from the canonical key's because H(pk) does); kosk_options::strict_encoding concerns proofs and is
 * not consulted.  Decapsulation has no branch and no address that depends on s, m', the comparison or z; its secret-derived scratch
 * (m', K-bar || coins, r, e1, e2, the rejection key) stays in the handle's HBM workspace until it is erased: by kosk_wipe_secrets, at the end of the
 * call under KOSK_WIPE_CALL, or by kosk_destroy.
 * All three calls run unmerged on the handle's own stream, reset and check the HIP error state like every entry point, and return -1
 * ("block limit", no results) if gen_matrix reached its block limit. */
#define KOSK_SS_BYTES 32
size_t kosk_ct_bytes(int kyber_k); /* KYBER_CIPHERTEXTBYTES 768 / 1088 / 1568; 0 outside 2..4 */
int kosk_kem_enc_batch(kosk_ctx *ctx, int n, const uint8_t *pk, const uint8_t *coins, uint8_t *ct, uint8_t *ss);
int kosk_kem_dec_batch(kosk_ctx *ctx, int n, const uint8_t *ct, const uint8_t *sk, uint8_t *ss);
/* The registrar's step: encapsulate to the public keys that the LAST COMPLETED verify call of at least n proofs left in HBM on this
 * handle (the rule of kosk_verify_resident_pk(pk == NULL)), and only where that call's verify bit is 1.  done[b] is that bit; ct and
 * ss of a rejected position are zero-filled; coins are consumed for every position, so the draw order does not depend on the outcome.
 * The public keys are decoded again from their resident bytes (the same result as reusing the verifier's t and A).  Needs
 * streams = 1.  -1 with a text when no verify call has completed, when the last one covered fewer than n proofs, was a
 * chunked kosk_verify_batch call (n > max_batch), verified with A and t from instances (kosk_verify_inst, or kosk_verify_resident after it: no pk bytes were decoded) or was followed
 * by a call that replaced the resident keys (a key generation, a verifier staging call in any wire format: image, compact (kosk_stage_verifier_inputs_compact, kosk_verify_batch_compact) or dense (kosk_stage_verifier_inputs_dense, kosk_verify_batch_dense)); and for a member of a cohort (combine >= 2): "not available with call combining". */
int kosk_kem_enc_verified(kosk_ctx *ctx, int n, const uint8_t *coins, uint8_t *ct, uint8_t *ss, uint8_t *done);

/* ---- KEM with one resident key (INTEGRATION.md 8.2 is the normative text): for a party that owns ONE ML-KEM key and answers many peers
 * with it.  kosk_kem_key_set loads one record -- exactly one of pk (kosk_pk_bytes) / sk (kosk_sk_bytes) non-NULL, host or device memory
 * -- into the handle's key slot: the pk bytes, A^T and H(pk) decoded once (one launch of k_kem_key_setup, synchronised), and for an sk
 * its s-hat, stored H(pk) and z.  The slot is its own HBM allocation (about 1.2 + 0.5 K^2 + 0.8 K KB), made at the first load; a handle
 * that never loads a key allocates nothing.  A second kosk_kem_key_set replaces the slot, the old one is wiped first;
 * kosk_kem_key_clear wipes and empties it.  Neither may be called while another thread is inside a call on the handle.
 * kosk_kem_key_state: KOSK_KEM_KEY_NONE / _PK / _SK; -1 for NULL.
 * kosk_kem_enc_key(n, coins) returns byte for byte what kosk_kem_enc_batch returns for n copies of the loaded pk record (loaded from an
 * sk: the pk inside it); kosk_kem_dec_key(n, ct) what kosk_kem_dec_batch returns for n copies of the loaded sk record.  Everything those
 * calls do holds: 12-bit fields >= q in t-hat / s-hat are folded mod q, decapsulation trusts the H(pk) stored in the sk and re-encrypts
 * with the pk inside it, the rejection key is SHAKE256(z || ct), encapsulation hashes the pk bytes as given; coins == NULL: one 32-byte
 * draw per item, in item order, on the caller's thread.  Buffers host or device memory, any n >= 1 in launch groups of 16384 items, which
 * do only the per-item work (no gen_matrix, no H(pk), no copy of the key).  Unmerged on the handle's own stream (a cohort member as for
 * kosk_kem_enc_batch); the HIP error state is reset and checked as in every entry point.  No branch and no address depends on s-hat,
 * m', the comparison or z.
 * -1 with a text and nothing started: NULL arguments, both or neither of pk / sk, n < 1, kosk_kem_enc_key on an empty slot,
 * kosk_kem_dec_key on a slot that is not in state SK.  -1 ("block limit"), the slot left empty, if gen_matrix reached its block limit
 * inside kosk_kem_key_set.
 * Erasure: s-hat and z are secret buffers of the inventory, the pk bytes, A^T and both H(pk) public ones.
 * kosk_wipe_secrets, kosk_kem_key_clear and kosk_destroy zero the secret part; after kosk_wipe_secrets a slot in state SK is in state PK,
 * kosk_kem_enc_key returns the same bytes as before and kosk_kem_dec_key returns -1 ("key was wiped") -- it never decapsulates with
 * zeros.  Under KOSK_WIPE_CALL the slot is a long-lived secret and NOT part of the wipe at the end of a call: that wipe clears the
 * per-call scratch (m', K-bar || coins, noise, rejection keys, ss) as before and leaves the slot alone, and kosk_kem_key_set keeps the
 * slot it just made. */
enum { KOSK_KEM_KEY_NONE = 0, KOSK_KEM_KEY_PK = 1, KOSK_KEM_KEY_SK = 2 };
int kosk_kem_key_set(kosk_ctx *ctx, const uint8_t *pk, const uint8_t *sk);
int kosk_kem_key_state(const kosk_ctx *ctx);
int kosk_kem_key_clear(kosk_ctx *ctx);
int kosk_kem_enc_key(kosk_ctx *ctx, int n, const uint8_t *coins, uint8_t *ct, uint8_t *ss);
int kosk_kem_dec_key(kosk_ctx *ctx, int n, const uint8_t *ct, uint8_t *ss);

/* ---- The verified-key registry (INTEGRATION.md 8.3 is the normative text): a table of admitted public keys in HBM, for a registrar that
 * talks to many enrolled peers again and again.  A key enters where a proof verified (kosk_registry_admit_verified) or where the caller
 * vouches for it (kosk_registry_admit); what depends on the key alone -- the pk bytes, SHA3-256 of them, A^T -- is computed once, at
 * admission (k_registry_admit); kosk_kem_enc_slots names a slot per item and does the per-item work only.
 * One registry per handle, on sub-context 0, in HBM allocations of its own (the KEM workspace may grow and move; the registry does not):
 * kosk_registry_slot_bytes per slot, about 2.9 / 5.8 / 9.8 KB for kyber_k 2 / 3 / 4 (0 for any other k).  A handle that never reserves
 * allocates nothing.  kosk_registry_reserve allocates exactly `capacity` empty slots; again only while no slot is occupied (the old
 * allocation is freed first); capacity 0 frees; -1 with a text for capacity < 0, a non-empty registry, or an allocation that fails (nothing is
 * left allocated then).  kosk_registry_level: occupied slots and capacity (0 / 0 without a registry); used / capacity may be NULL.
 * slots: n int32 values in HOST memory.  A value outside [0, capacity) makes any of these calls return -1 with a text and nothing started;
 * so does a value named twice within one kosk_registry_admit* call.  Repeats are fine in kosk_registry_evict, kosk_registry_read and
 * kosk_kem_enc_slots (many items to one peer is the normal case).
 * kosk_registry_admit_verified: key b of the LAST COMPLETED verify call of at least n proofs goes into slots[b], only where that call's verify
 * bit is 1; done[b] (host memory) is that bit; where it is 0 the named slot is not touched and keeps an earlier key.  The preconditions and
 * refusals are those of kosk_kem_enc_verified, and the keys are decoded from their resident bytes as there.
 * kosk_registry_admit: the same for n pk records (host or device memory) that THE CALLER VOUCHES FOR -- the library has not seen a proof
 * for them; accept: n bytes of host memory, 0 = leave the slot alone, or NULL for all.  For verdicts of a cohort member's merged run, of a
 * chunked kosk_verify_batch, or of another handle; works on a cohort member, unmerged.  No encoding check: 12-bit fields >= q are folded
 * as in kosk_kem_enc_batch (run kosk_kem_check_pk first for FIPS 203's modulus check).
 * Admitting into an occupied slot replaces its key.  -1 ("block limit") if gen_matrix reached its block limit inside an admitting call: the
 * slots that call wrote are left empty, every other slot is untouched.
 * kosk_registry_evict zeroes the named slots' records and flags; an empty slot stays as it is.  kosk_registry_read (audits, tests):
 * state[b] (host memory) 0 or 1; pk / h: NULL, or n records of kosk_pk_bytes / 32 bytes, host or device memory, zeros for an empty slot.
 * kosk_kem_enc_slots: for every b with an occupied slots[b], ct and ss equal byte for byte what kosk_kem_enc_batch returns for the pk
 * record admitted to that slot with the same coins (fields >= q folded, H(pk) over the bytes as given).  done[b] is the slot's occupancy
 * (host or device memory); ct and ss of an empty slot are zero-filled; coins are consumed for every position (coins == NULL: one 32-byte
 * draw per item, in item order, on the caller's thread, whatever done says).  Any n >= 1 in launch groups of 16384 items, buffers host or
 * device memory, unmerged on the handle's own stream, also on a cohort member.
 * No registry call touches the prover's or verifier's resident state, the bank, the one-key slot or the fail masks.
 * Erasure: the registry's buffers are public buffers of the inventory: kosk_secret_scan covers them, kosk_wipe_secrets and
 * the wipe at the end of a call under KOSK_WIPE_CALL leave them alone; the per-call scratch of kosk_kem_enc_slots (coins, K-bar || coins,
 * noise, ss) is secret as for kosk_kem_enc_batch.  kosk_destroy and kosk_registry_reserve(0) free the registry.
 * reserve, admit* and evict must not be called while another thread is inside a call on the handle (the rule of kosk_kem_key_set). */
size_t kosk_registry_slot_bytes(int kyber_k);
int kosk_registry_reserve(kosk_ctx *ctx, int capacity);
int kosk_registry_level(const kosk_ctx *ctx, int *used, int *capacity);
int kosk_registry_admit_verified(kosk_ctx *ctx, int n, const int32_t *slots, uint8_t *done);
int kosk_registry_admit(kosk_ctx *ctx, int n, const uint8_t *pk, const uint8_t *accept, const int32_t *slots);
int kosk_registry_evict(kosk_ctx *ctx, int n, const int32_t *slots);
int kosk_registry_read(kosk_ctx *ctx, int n, const int32_t *slots, uint8_t *state, uint8_t *pk, uint8_t *h);
int kosk_kem_enc_slots(kosk_ctx *ctx, int n, const int32_t *slots, const uint8_t *coins, uint8_t *ct, uint8_t *ss, uint8_t *done);

/* ---- The registry by fingerprint (INTEGRATION.md 8.4 is the normative text): the index beside the keys.  A peer is known by
 * SHA3-256(pk), which every slot stores as h; an open-addressing table over those fingerprints in HBM lets the library look keys up, refuse
 * keys that are enrolled already, and pick the slots.
 * The index: T = kosk_registry_index_entries(capacity) = the smallest power of two >= 2 x capacity int32 entries (0 for capacity < 1), one more
 * allocation of the registry (a public buffer, slot numbers only), made at the first of the calls below and freed with the registry; a
 * registry that never uses them allocates what it allocated before.  kosk_registry_index_home(capacity, h) = LE32(h[0..4)) & (T - 1) is a
 * fingerprint's home entry (-1 for capacity < 1 or NULL); probing is linear.  One entry per distinct fingerprint among the occupied slots,
 * holding the LOWEST such slot (the admit calls above may put equal keys into several slots).  Every reserve / admit / evict / enrol
 * invalidates the index and the next call below rebuilds it on the GPU (k_registry_index); no unsalted-hash attack applies beyond a probe
 * chain as long as the keys the attacker itself enrolled (8.4).
 * kosk_registry_find: h = n x 32 bytes, slots = n int32, each host or device memory of any alignment; slots[b] = the lowest occupied slot
 * whose stored H(pk) equals h[b], or -1.  Any n >= 1 in launch groups of 16384; works on a cohort member, unmerged.
 * kosk_registry_enrol_verified / kosk_registry_enrol: the candidates and preconditions of kosk_registry_admit_verified /
 * kosk_registry_admit, but the library picks the slots: slots (n int32) and status (n bytes) are OUTPUTS in host memory.  Positions are
 * taken in ascending b.  A position whose verify bit / accept byte is 0 is KOSK_ENROL_REJECTED, slot -1, and does not count as an occurrence
 * of its key.  A position whose fingerprint is in the registry already, or was admitted at a lower position of this call, is
 * KOSK_ENROL_DUPLICATE; slots[b] is the slot that holds the key; nothing is written for it.  Every other position is KOSK_ENROL_ADMITTED
 * into the lowest-numbered empty slot not yet given out in this call.  More new keys than empty slots: -1 ("registry is full"), nothing
 * changed.  Equality is equality of the pk BYTES: two encodings of one key (12-bit fields >= q) are two fingerprints; the strict verifier
 * refuses proofs over such a pk anyway, and a caller of kosk_registry_enrol who cares runs kosk_kem_check_pk first.  -1 ("block limit")
 * as for kosk_registry_admit: the slots this call wrote are emptied.
 * kosk_kem_enc_peers: kosk_kem_enc_slots with the lookup on the GPU in front of the per-item kernels; no slot number crosses to the host.
 * h: n x 32 bytes, host or device memory.  For every b whose fingerprint is found, ct and ss are byte for byte those of kosk_kem_enc_slots
 * on kosk_registry_find's slot with the same coins; done[b] = found (host or device memory); ct and ss of a miss are zero-filled; coins are
 * consumed for every position (coins == NULL: one 32-byte draw per item, in item order, on the caller's thread; a refused call draws none).
 * Refusals (-1, a text that begins with the call's name, nothing started): NULL arguments, n < 1, no registry reserved.
 * Erasure: the index holds slot numbers only; the staged query fingerprints and candidate records are zeroed before each of these calls
 * returns; kosk_wipe_secrets and KOSK_WIPE_CALL leave the index alone, as they leave the registry. */
size_t kosk_registry_index_entries(int capacity);
int kosk_registry_index_home(int capacity, const uint8_t h[32]);
int kosk_registry_find(kosk_ctx *ctx, int n, const uint8_t *h, int32_t *slots);
enum { KOSK_ENROL_REJECTED = 0, KOSK_ENROL_ADMITTED = 1, KOSK_ENROL_DUPLICATE = 2 };
int kosk_registry_enrol_verified(kosk_ctx *ctx, int n, int32_t *slots, uint8_t *status);
int kosk_registry_enrol(kosk_ctx *ctx, int n, const uint8_t *pk, const uint8_t *accept, int32_t *slots, uint8_t *status);
int kosk_kem_enc_peers(kosk_ctx *ctx, int n, const uint8_t *h, const uint8_t *coins, uint8_t *ct, uint8_t *ss, uint8_t *done);

/* ---- The registry tree, format kosk-regtree-v1 (INTEGRATION.md 8.5 is the normative text): a Merkle tree over the slots' fingerprints, built
 * and kept current on the GPU beside the registry.  Out of it come a 32-byte root that pins the whole table, and per-key inclusion paths that
 * anyone checks with kosk_regtree_root_from_path, on the host, without a handle.  A path for an empty slot proves that the slot is empty.
 * TAG = the 15 ASCII bytes "kosk-regtree-v1"; every hash is SHA3-256 of one rate block:
 *   leaf of an occupied slot   L(h)   = SHA3-256(TAG || 00 || h[32] || LE32(kyber_k))     h = the slot's stored SHA3-256(pk)
 *   leaf of an empty slot      E      = SHA3-256(TAG || 01 || LE32(kyber_k))
 *   inner node                 N(l,r) = SHA3-256(TAG || 02 || l[32] || r[32])
 * D = kosk_registry_tree_depth(capacity) is the smallest D with 2^D >= capacity (0 for capacity 1, -1 for capacity < 1), P = 2^D.  Level 0
 * has P leaves: L(h_s) for an occupied slot s < capacity, E for an empty slot and for every padding position s >= capacity; node i of level
 * l + 1 is N(level_l[2i], level_l[2i + 1]); the root is the one node of level D (for D = 0: leaf 0).  The path of slot s is D records of 32
 * bytes, level 0 first, record l = node (s >> l) ^ 1 of level l; walking up from the leaf, step l computes N(path[l], cur) if bit l of s is
 * set, else N(cur, path[l]).  The root binds neither capacity nor the occupied count: kosk_registry_root returns them beside it for a signed
 * tree head.  Equal keys in several slots (kosk_registry_admit) give equal leaves; lookup by fingerprint names the lowest slot.  Proofs of
 * ABSENCE of a fingerprint come from the sorted tree, kosk-regsort-v1, below.
 * Host functions: kosk_registry_tree_bytes = (2P - 1) * 32, the HBM the tree takes (0 for capacity < 1).  kosk_regtree_leaf (h == NULL: E)
 * and kosk_regtree_node: -1 for kyber_k outside 2..4 or a NULL argument.  kosk_regtree_root_from_path: the root that (slot, h or NULL for
 * "empty", path[depth][32]) implies -- the caller compares it with the published root; -1: bad k, depth outside 0..31, slot outside
 * [0, 2^depth), NULL root, NULL path with depth > 0.  Pointers of any alignment.
 * On a handle: the tree is one more allocation of the registry (with a list of subtree numbers and, from the first proving call on, a
 * staging buffer for paths), made by the first of the calls below and freed with the registry; a registry that never asks allocates and
 * launches what it did before.  Every admit / evict / enrol marks the leaf subtrees (KOSK_REGTREE_TIER_LEVELS = 10 levels, 1 024 slots)
 * of the slots it writes, and the first tree call after a mutation rehashes those subtrees and the levels above them (k_registry_tree); a tree
 * call on a current tree launches nothing but the gather (k_registry_path).
 * kosk_registry_root: root = 32 bytes of host or device memory; used / capacity may be NULL.
 * kosk_registry_prove_slots: slots = n int32 in HOST memory, repeats are fine, a value outside [0, capacity) returns -1 and starts nothing;
 * state[b] (host memory) = occupancy; h: NULL, or n x 32 bytes, the stored fingerprints, zeros for an empty slot; paths: n x D x 32 bytes
 * (may be NULL when D = 0); root: NULL, or the root the paths belong to, taken from the same tree state.  h, paths and root may be host or
 * device memory of any alignment.  An empty slot gets a valid path: it checks with h == NULL in kosk_regtree_root_from_path.
 * kosk_registry_prove_peers: h = n x 32 query fingerprints; the lookup runs on the GPU (k_registry_find) in front of the gather; slots[b] =
 * the lowest occupied slot that holds the fingerprint, or -1; done[b] = found; a miss gets a zero-filled path.  h, slots, done, paths and root
 * may be host or device memory.
 * Both: any n >= 1 in launch groups of 16384, unmerged on the handle's own stream, also on a cohort member.  Refusals (-1, a text that begins
 * with the call's name, nothing started): NULL required arguments, n < 1, no registry reserved.  No call here touches the prover's or
 * verifier's resident state, the bank, the one-key slot, the fail masks, the registry's slots, or the validity of the fingerprint index
 * (kosk_registry_prove_peers builds a stale index as kosk_registry_find does).
 * Erasure: the tree, the subtree list and the path staging are public buffers of the inventory: kosk_secret_scan covers
 * them, kosk_wipe_secrets and KOSK_WIPE_CALL leave them alone; the staged query fingerprints are zeroed before kosk_registry_prove_peers
 * returns.  After an eviction the evicted key's leaf and its ancestors stay in the tree until the next tree call rebuilds them: hashes of a
 * public fingerprint, not the fingerprint. */
enum { KOSK_REGTREE_TIER_LEVELS = 10 };
int kosk_registry_tree_depth(int capacity);
size_t kosk_registry_tree_bytes(int capacity);
int kosk_regtree_leaf(int kyber_k, const uint8_t *h, uint8_t out[32]);
int kosk_regtree_node(const uint8_t l[32], const uint8_t r[32], uint8_t out[32]);
int kosk_regtree_root_from_path(int kyber_k, int depth, int32_t slot, const uint8_t *h, const uint8_t *path, uint8_t root[32]);
int kosk_registry_root(kosk_ctx *ctx, uint8_t root[32], int *used, int *capacity);
int kosk_registry_prove_slots(kosk_ctx *ctx, int n, const int32_t *slots, uint8_t *state, uint8_t *h, uint8_t *paths, uint8_t *root);
int kosk_registry_prove_peers(kosk_ctx *ctx, int n, const uint8_t *h, int32_t *slots, uint8_t *paths, uint8_t *done, uint8_t *root);

/* ---- The sorted tree, format kosk-regsort-v1 (INTEGRATION.md 8.6 is the normative text): a second Merkle tree over the registry, its leaves
 * the occupied slots' (fingerprint, slot) pairs in ascending order.  Two adjacent leaves that straddle a fingerprint prove that it is NOT
 * enrolled; anyone checks such a proof with kosk_regsort_check_proof, on the host, without a handle.
 * TAG = the 15 ASCII bytes "kosk-regsort-v1"; every hash is SHA3-256 of one rate block:
 *   key leaf       S(h, slot) = SHA3-256(TAG || 00 || h[32] || LE32(slot) || LE32(kyber_k))
 *   padding leaf   Z          = SHA3-256(TAG || 01 || LE32(kyber_k))
 *   inner node     N(l, r)    = SHA3-256(TAG || 02 || l[32] || r[32])
 * One entry (h, slot) per occupied slot, m = used of them (equal keys in several slots give several entries), ascending by h as 32 bytes in
 * memcmp order, then by slot: the order is total and the sequence unique.  D = kosk_registry_tree_depth(capacity), P = 2^D; position i < m
 * holds S of the i-th entry, positions m .. P - 1 hold Z; levels, paths (record l of position p = node (p >> l) ^ 1 of level l) and the walk
 * are those of the slot tree with this section's N.
 * Rank of a query x: lb = the number of entries with h < x.  x is PRESENT iff lb < m and entry lb has h == x (the lowest slot that holds x,
 * the rule of kosk_registry_find), else ABSENT.  The left neighbour is position lb - 1 (exists iff lb >= 1), the right neighbour position
 * lb (exists iff lb < P; a key leaf iff lb < m, else Z).
 * The proof record, kosk_regsort_proof_bytes(D) = 16 + 64 + 64 D bytes (0 for D outside 0..31), integers LE32:
 *    0 pos_l (-1: no left record)   4 slot_l   8 slot_r (0 if Z or none)
 *   12 flags: bit0 left record present, bit1 right record present, bit2 right is a key leaf, bit3 PRESENT
 *   16 h_l[32]   48 h_r[32]   80 path_l[D][32]   80 + 32 D path_r[D][32]        (unused parts are zero)
 * PRESENT: bits 0 and 3, h_l == x, pos_l = lb, the right half zero.
 * kosk_regsort_check_proof: 2 = PRESENT (h_l == x, 0 <= pos_l < P, the left walk gives root); 1 = ABSENT (bit3 clear, at least one record;
 * with a left record 0 <= pos_l < P, h_l < x and its walk gives root, without one pos_l == -1; with a right record pos_l + 1 < P and at
 * position pos_l + 1 either bit2, x < h_r and the walk of S(h_r, slot_r) gives root, or no bit2 and the walk of Z gives root, without one
 * pos_l == P - 1); 0 = the record proves neither (any other flag pattern, bits above bit3); -1 = bad kyber_k, depth outside 0..31, a NULL
 * argument.  The root binds the sorted sequence of (fingerprint, slot) pairs; an ABSENT verdict is sound against a registrar whose tree is
 * well formed (sorted, padding at the end), which one record cannot show: an auditor who holds the table recomputes the root (one host sort
 * and 2P hashes).  A signed head carries both roots, used and capacity.
 * kosk_regsort_leaf (h == NULL: Z), kosk_regsort_node, kosk_regsort_root_from_path (pos, h or NULL for Z, slot, path[depth][32]): -1 as
 * their kosk_regtree_* counterparts, and for a key leaf with slot < 0.  Pointers of any alignment.
 * On a handle: the sorted records, the tree and (from the first proving call on) four staging buffers are public allocations of the
 * registry, made by the first call below and freed with it; a registry that never asks allocates and launches what it did before.  Every
 * admit / evict / enrol marks the sorted tree stale, and the first call below after a mutation rebuilds it whole: a bitonic sort of P
 * 16-byte records (k_regsort_keys, k_regsort_tile: tiles of 2 048 in LDS, k_regsort_step above the tile), then the tiers (k_regsort_tree).
 * kosk_registry_sorted_root: root = 32 bytes of host or device memory; used / capacity may be NULL.
 * kosk_registry_prove_absent: h = n x 32 query fingerprints; kind[b] = 1 (ABSENT) or 2 (PRESENT); records = n x proof_bytes(D); root: NULL,
 * or the root the records belong to.  Every query gets a valid record of one kind or the other.  Every pointer may be host or device memory
 * of any alignment.  Any n >= 1 in launch groups of 16384, unmerged on the handle's own stream, also on a cohort member.  Refusals, the
 * thread rule and the erasure rule are those of the slot tree: -1 for NULL required arguments, n < 1, no registry reserved; the buffers are
 * public entries of the inventory; the staged queries are zeroed before the call returns.  After an eviction the sorted records keep the
 * evicted key's 8-byte prefix and slot until the next call here rebuilds them.
 * kosk_regsort_order_device: a kernel-level entry point that needs no registry and runs exactly the sort kernels of the rebuild: n records of
 * 32 bytes (d_h, 8-byte aligned) and n flag bytes in DEVICE memory give d_order[i] = the index of the i-th entry in order for i < m (the
 * number of non-zero flags), -1 from m on.  -1: NULL arguments, n < 1, n > 2^24, a misaligned pointer. */
size_t kosk_regsort_proof_bytes(int depth);
int kosk_regsort_leaf(int kyber_k, const uint8_t *h, int32_t slot, uint8_t out[32]);
int kosk_regsort_node(const uint8_t l[32], const uint8_t r[32], uint8_t out[32]);
int kosk_regsort_root_from_path(int kyber_k, int depth, int32_t pos, const uint8_t *h, int32_t slot, const uint8_t *path, uint8_t root[32]);
int kosk_regsort_check_proof(int kyber_k, int depth, const uint8_t x[32], const uint8_t *record, const uint8_t root[32]);
int kosk_registry_sorted_root(kosk_ctx *ctx, uint8_t root[32], int *used, int *capacity);
int kosk_registry_prove_absent(kosk_ctx *ctx, int n, const uint8_t *h, uint8_t *kind, uint8_t *records, uint8_t *root);
int kosk_regsort_order_device(kosk_ctx *ctx, int n, const uint8_t *d_h, const uint8_t *d_flag, int32_t *d_order);

/* ---- The registry history, format kosk-reghist-v1 (INTEGRATION.md 8.7 is the normative text): an append-only Merkle tree over the
 * registry's mutation events, kept current in HBM by the mutating calls themselves, with checkpoints that bind the two state roots into it,
 * inclusion proofs for events and consistency proofs between any two sizes.  It is the third leg beside inclusion (8.5) and absence (8.6):
 * a peer that holds two signed heads checks that the later history extends the earlier one.
 * TAG = the 15 ASCII bytes "kosk-reghist-v1"; every hash is SHA3-256 of one rate block:
 *   event leaf       V = SHA3-256(TAG || 00 || h[32] || LE32(op) || LE32(slot) || LE32(kyber_k))
 *   checkpoint leaf  C = SHA3-256(TAG || 01 || slot_root[32] || sorted_root[32] || LE32(used) || LE32(capacity) || LE32(kyber_k))
 *   inner node       N(l, r) = SHA3-256(TAG || 02 || l[32] || r[32])
 *   empty history    O = SHA3-256(TAG || 03 || LE32(kyber_k))
 * The stored event record, KOSK_REGHIST_EVENT_BYTES = 80 bytes: 0 LE32 op; 4 LE32 a (ops 1 / 2: the slot; op 3: used); 8 LE32 b (0;
 * capacity); 12 LE32 zero; 16 x[32] (the fingerprint h, of the evicted key for op 2; slot_root); 48 y[32] (zeros; sorted_root).
 * The tree over the first n leaves has the shape of RFC 6962: H(0) = O, H of one leaf is that leaf's hash, and for n > 1 with s the largest
 * power of two below n, H(D[0:n]) = N(H(D[0:s]), H(D[s:n])).  Node (l, i) is complete at size n iff (i + 1) 2^l <= n; it covers leaves
 * [i 2^l, (i + 1) 2^l) and never changes.  R_l is the hash of the trailing leaves [(n >> l) << l, n) where there are any.
 * Inclusion path of leaf i at size n: l = 0, idx = i; while level l has more than one node (n >> l complete ones and one ragged node iff
 * n & (2^l - 1) != 0): emit node (l, idx ^ 1) if it is complete, R_l if idx ^ 1 == n >> l and there is a ragged node, nothing otherwise; then
 * l += 1, idx >>= 1.  At most depth(n) records.  Consistency proof from m to n, 0 < m < n: l = the trailing zero bits of m, idx = (m - 1) >> l;
 * emit node (l, idx) first if idx != 0, then the records of the walk above from (l, idx).  At most depth(n) + 1 records; empty for m == n
 * and m == 0.
 * A proof record: four LE32 (count; index or old_size; size; 0), `count` records of 32 bytes, zero padding to kosk_reghist_path_bytes(size)
 * = 16 + 32 depth(size) or kosk_reghist_consistency_bytes(size) = 16 + 32 (depth(size) + 1) bytes (both 0 for size < 1).
 * kosk_reghist_depth: the smallest d with 2^d >= size; 0 for size 0 or 1; -1 for size < 0.
 * kosk_reghist_leaf: the leaf of a stored record; -1: bad k, NULL, op outside 1..3, a non-zero reserved field (b and y of ops 1 / 2, word 12).
 * kosk_reghist_root_from_path: fn = index, sn = size - 1, r = leaf; per record v: fail if sn == 0; if fn is odd or fn == sn, r = N(v, r) and,
 * if fn is even, both shift right until fn is odd or zero; otherwise r = N(r, v); then both shift right by one.  0 with the root written iff
 * sn == 0 at the end; -1: malformed (also: a header that disagrees with the arguments, a count above depth(size), non-zero padding).
 * kosk_reghist_check_consistency: 1 consistent / 0 not / -1 bad arguments (NULL, a negative size, old_size > size, size < 1).  m == 0:
 * consistent iff count == 0 (root_old is not read); m == n: iff count == 0 and the roots are equal.  Otherwise root_m goes in front of the
 * proof if m is a power of two; fn = m - 1, sn = n - 1, both shifted right while fn is odd; fr = sr = proof[0]; per further record v: fail
 * if sn == 0; if fn is odd or fn == sn, fr = N(v, fr), sr = N(v, sr) and, if fn is even, both shift right until fn is odd or zero; otherwise
 * sr = N(sr, v); then both shift right by one.  Consistent iff sn == 0, fr == root_m, sr == root_n.  A header that disagrees with the
 * arguments, a count above the bound and non-zero padding give 0.  All host functions: no handle, no GPU, pointers of any alignment.
 * Which events a call appends (decided on the host from the occupancy mirror before anything runs): an admitting call
 * (kosk_registry_admit, _admit_verified, _enrol, _enrol_verified) appends one EVICT(slot, old fingerprint) per accepted position whose slot
 * is occupied, in ascending position, then one ADMIT(slot, new fingerprint) per accepted position, in ascending position; masked, REJECTED
 * and DUPLICATE positions append nothing.  kosk_registry_evict appends one EVICT per occupied slot at its first occurrence in the call.
 * An admitting call that fails with "block limit" has emptied the slots it wrote: its events are the EVICT events of the positions in the
 * launch groups that were started.  Replaying events 0 .. size - 1 onto an empty table gives the table's (slot, fingerprint) content.  A
 * call whose events do not fit is refused with -1 ("history is full"), nothing changed.
 * On a handle.  kosk_registry_history_reserve: needs a reserved registry with no occupied slot; max_events 1 .. 2^24; allowed again only
 * while size == 0; 0 frees at any time; kosk_registry_reserve frees the history with the registry.  The events, the complete nodes
 * (level-major), 33 ragged-node slots, a job list and (from the first proving call on) staging are public allocations of the registry; a
 * registry without a history allocates and launches what it did before.  kosk_registry_history_head: the root at any size <= the current
 * one (< 0: current), size 0 gives O; root = host or device memory.  kosk_registry_history_checkpoint: brings both state trees up to date
 * (their counters move as for kosk_registry_root and kosk_registry_sorted_root) and appends one op-3 event whose roots are read in HBM;
 * *index = the event's position.  kosk_registry_history_read: n raw records from `first` on to host or device memory.
 * kosk_registry_history_prove_events / _prove_consistency: index / old_size = n int32 in HOST memory; size < 0: the current size; an index
 * outside [0, size), an old size outside [0, size] or a size above the current one returns -1 and starts nothing; leaves (n x 32) and root
 * may be NULL; every output may be host or device memory of any alignment; any n >= 1 in launch groups of 16384, unmerged on the handle's
 * own stream, also on a cohort member.  Refusals return -1 with a text that begins with the call's name, and nothing is started; calls that
 * may append follow the thread rule of kosk_registry_reserve, kosk_registry_admit* and kosk_registry_evict.
 * Erasure: the buffers are public entries of the inventory: kosk_secret_scan covers them, kosk_wipe_secrets and
 * KOSK_WIPE_CALL leave them alone.  With a history reserved the fingerprint of an evicted key STAYS in HBM on purpose: a public log
 * remembers.  A registrar who needs "no byte of the key is left" (8.3) does not reserve a history. */
enum { KOSK_REGHIST_ADMIT = 1, KOSK_REGHIST_EVICT = 2, KOSK_REGHIST_CHECKPOINT = 3 };
enum { KOSK_REGHIST_TIER_LEVELS = 10 };
#define KOSK_REGHIST_EVENT_BYTES 80
int kosk_reghist_depth(int size);
size_t kosk_reghist_path_bytes(int size);
size_t kosk_reghist_consistency_bytes(int size);
int kosk_reghist_leaf(int kyber_k, const uint8_t event[80], uint8_t out[32]);
int kosk_reghist_node(const uint8_t l[32], const uint8_t r[32], uint8_t out[32]);
int kosk_reghist_empty_root(int kyber_k, uint8_t out[32]);
int kosk_reghist_root_from_path(int index, int size, const uint8_t leaf[32], const uint8_t *record, uint8_t root[32]);
int kosk_reghist_check_consistency(int old_size, int size, const uint8_t root_old[32], const uint8_t root_new[32], const uint8_t *record);
int kosk_registry_history_reserve(kosk_ctx *ctx, int max_events);
int kosk_registry_history_level(const kosk_ctx *ctx, int *size, int *max_events);
int kosk_registry_history_head(kosk_ctx *ctx, int size, uint8_t root[32], int *size_out);
int kosk_registry_history_checkpoint(kosk_ctx *ctx, int *index);
int kosk_registry_history_read(kosk_ctx *ctx, int first, int n, uint8_t *events);
int kosk_registry_history_prove_events(kosk_ctx *ctx, int size, int n, const int32_t *index, uint8_t *leaves, uint8_t *records, uint8_t *root);
int kosk_registry_history_prove_consistency(kosk_ctx *ctx, int size, int n, const int32_t *old_size, uint8_t *records, uint8_t *root);

/* ---- The registry monitor (INTEGRATION.md 8.8 is the normative text): the third role of the transparency log.  A monitor takes the stored
 * event log of a registrar (kosk_registry_history_read) and checks that the events replay cleanly onto an empty table and that, at every
 * checkpoint, the slot root, the sorted root, used and capacity that the registrar bound into the log are those of the replayed table.
 * A monitor is optional state on a handle, independent of the handle's registry (one handle may hold both): capacity x (a 32-byte
 * fingerprint and a flag byte) -- no pk bytes, no A^T --, a slot tree (8.5) and a sorted tree (8.6) over that table, and the complete nodes
 * and 33 ragged slots of a history tree (8.7) over the events fed so far.  It keeps no event records: 32 bytes of HBM per event.
 * kosk_monitor_reserve: capacity as for kosk_registry_reserve (>= 1), max_events 1 .. 2^24; allowed at any time, a second call starts a
 * fresh, empty replay; (0, 0) frees; -1 with a text for anything else or an allocation that fails (no monitor is left then).
 * kosk_monitor_level: events replayed, max_events, occupied slots, capacity, failed (all 0 without a monitor); any pointer may be NULL.
 * kosk_monitor_feed: the next n >= 1 stored event records of KOSK_REGHIST_EVENT_BYTES each, in log order, host or device memory of any
 * alignment.  1: all n were accepted and size has grown by n.  0: the log is invalid; *bad_index = the absolute index of the LOWEST invalid
 * event, *reason = its lowest-numbered reason (both may be NULL).  -1 with a text that begins with the call's name and nothing started:
 * NULL, n < 1, no monitor, size + n > max_events ("monitor is full"), a monitor that has failed.
 * The replay rule.  BAD_RECORD: op outside 1..3 or a reserved field that is not zero (the fields kosk_reghist_leaf rejects); BAD_SLOT: an
 * ADMIT or EVICT with a >= capacity.  An event on slot s sees the state implied by the latest earlier event on s among all events fed so
 * far -- an ADMIT leaves s occupied with that event's x, an EVICT leaves it empty, no earlier event means empty -- whether or not that
 * earlier event was itself valid.  ADMIT_OCCUPIED: an ADMIT on an occupied slot; EVICT_EMPTY: an EVICT on an empty slot; EVICT_MISMATCH:
 * an EVICT whose x differs from the stored 32 bytes.  A CHECKPOINT is checked in this order, the first failure is the reason: a against the
 * number of occupied slots (CP_USED), b against capacity (CP_CAPACITY), x against the slot tree's root of the replayed table
 * (CP_SLOT_ROOT), y against the sorted tree's root (CP_SORTED_ROOT); the comparison runs on the device, no root crosses to the host.
 * After a rejection the monitor is FAILED: kosk_monitor_level reports failed = 1 and a size <= bad_index; the table, both roots and
 * kosk_monitor_head(size) are exactly those of events [0, size); every later kosk_monitor_feed returns -1 until kosk_monitor_reserve.  How
 * far below bad_index the size lands is the implementation's segmentation and is not specified.
 * kosk_monitor_head: the history root at any size <= the current one (< 0: current; size 0 gives O), as kosk_registry_history_head.
 * kosk_monitor_roots: brings both state trees up to date and returns their roots; either pointer may be NULL.  kosk_monitor_read:
 * kosk_registry_read without the pk; state = host memory, h = NULL or n x 32 bytes, zeros for an empty slot.  root, slot_root,
 * sorted_root and h may be host or device memory.
 * All calls run unmerged on the handle's own stream, also on a cohort member; reserve and feed follow the thread rule of
 * kosk_registry_reserve, kosk_registry_admit* and kosk_registry_evict.  No monitor call touches the handle's registry, and no registry call
 * the monitor: kosk_registry_reserve leaves it alone.  A handle that never reserves a monitor allocates and launches what it did before.
 * Erasure: the monitor's buffers are public entries of the inventory (a log is public): kosk_secret_scan covers them,
 * kosk_wipe_secrets and KOSK_WIPE_CALL leave them alone.  kosk_destroy and kosk_monitor_reserve(0, 0) free them. */
enum { KOSK_MONITOR_OK = 0, KOSK_MONITOR_BAD_RECORD = 1, KOSK_MONITOR_BAD_SLOT = 2, KOSK_MONITOR_ADMIT_OCCUPIED = 3, KOSK_MONITOR_EVICT_EMPTY = 4,
       KOSK_MONITOR_EVICT_MISMATCH = 5, KOSK_MONITOR_CP_USED = 6, KOSK_MONITOR_CP_CAPACITY = 7, KOSK_MONITOR_CP_SLOT_ROOT = 8, KOSK_MONITOR_CP_SORTED_ROOT = 9 };
int kosk_monitor_reserve(kosk_ctx *ctx, int capacity, int max_events);
int kosk_monitor_level(const kosk_ctx *ctx, int *size, int *max_events, int *used, int *capacity, int *failed);
int kosk_monitor_feed(kosk_ctx *ctx, int n, const uint8_t *events, int *bad_index, int *reason);
int kosk_monitor_head(kosk_ctx *ctx, int size, uint8_t root[32], int *size_out);
int kosk_monitor_roots(kosk_ctx *ctx, uint8_t slot_root[32], uint8_t sorted_root[32]);
int kosk_monitor_read(kosk_ctx *ctx, int n, const int32_t *slots, uint8_t *state, uint8_t *h);

/* ---- The relying party (INTEGRATION.md 8.9 is the normative text): the role the log exists for.  A relying party holds a signed history
 * head, has checked a checkpoint event's inclusion under it on the host (kosk_reghist_root_from_path) and taken slot_root and sorted_root
 * from that event; peers then send their public keys with proofs under those roots.  It has no registry: these calls need no registry,
 * monitor or history on the handle and touch none.  All items of a call are checked against ONE root; kyber_k is the handle's.
 * kosk_regtree_check_paths: ok[b] = 1 iff kosk_regtree_root_from_path(kyber_k, depth, slots[b], state[b] ? h + 32 b : NULL, paths_b, r)
 * returns 0 and r equals root, else 0 -- a slot outside [0, 2^depth) gives 0.  paths: n x depth x 32 bytes (may be NULL when depth = 0);
 * state: NULL (every item claims "occupied, fingerprint h[b]") or n bytes, a zero byte claims "slot b is empty" and h[b] is ignored; h may
 * be NULL only if state is given and all zero (an "occupied" claim without fingerprints gives 0).
 * kosk_regsort_check_proofs: verdict[b] = exactly what kosk_regsort_check_proof(kyber_k, depth, x_b, record_b, root) returns: 0, 1 (ABSENT)
 * or 2 (PRESENT).  x: n x 32 bytes; records: n x kosk_regsort_proof_bytes(depth).
 * kosk_kem_enc_proven: pk = n records of kosk_pk_bytes; the call computes h_b = SHA3-256(pk_b) on the device, over the bytes as given;
 * done[b] = the verdict of kosk_regtree_check_paths for (slots[b], occupied, h_b, paths_b); where done[b] = 1, ct and ss are byte for byte
 * those of kosk_kem_enc_batch on pk_b with the same coins (fields >= q fold as there); where done[b] = 0 they are zero-filled, as for a miss
 * of kosk_kem_enc_peers.  The verdict reaches the encapsulation as its mask in HBM: no key whose path fails gets a ciphertext, and no
 * verdict crosses to the host in between.  Coins are consumed for every position: with coins == NULL one 32-byte draw per item, in item
 * order, on the caller's thread; a refused call draws none.  "block limit" behaves as for kosk_kem_enc_batch.
 * Any n >= 1, in launch groups of 16384; unmerged on the handle's own stream, also on a cohort member.  Every array may be host or device
 * memory of any alignment; slots too (untrusted peer data, not inspected on the host).  -1 with a text that begins with the call's name and
 * nothing started: a NULL required argument, n < 1, depth outside 0..31.  Whatever a peer could have sent wrong is a verdict, never a
 * refusal.
 * Erasure: the staging buffers (paths and proof records, fingerprints, slots, claims, verdicts) are public entries of
 * the inventory, made at the first of these calls: kosk_secret_scan covers them, kosk_wipe_secrets and KOSK_WIPE_CALL leave them alone.  The
 * per-call scratch of kosk_kem_enc_proven (coins, K-bar || coins, noise, ss) is secret exactly as for kosk_kem_enc_batch.  A handle that
 * never makes one of these calls allocates and launches what it did before. */
int kosk_regtree_check_paths(kosk_ctx *ctx, int n, int depth, const int32_t *slots, const uint8_t *state, const uint8_t *h, const uint8_t *paths, const uint8_t root[32], uint8_t *ok);
int kosk_regsort_check_proofs(kosk_ctx *ctx, int n, int depth, const uint8_t *x, const uint8_t *records, const uint8_t root[32], uint8_t *verdict);
int kosk_kem_enc_proven(kosk_ctx *ctx, int n, int depth, const uint8_t *pk, const int32_t *slots, const uint8_t *paths, const uint8_t root[32], const uint8_t *coins, uint8_t *ct, uint8_t *ss, uint8_t *done);

/* ---- Signed heads, format kosk-headsig-v1 (INTEGRATION.md 8.10 is the normative text): the registrar's signature over a history head, so
 * that the trust chain of 8.9 starts from a public key and needs nothing from outside this library.  Winternitz one-time signatures
 * (w = 8, 34 chains of 255 steps) under a Merkle tree of 2^height one-time keys, the construction of LMS (RFC 8554) over SHAKE256 with
 * 32-byte outputs; the records are this project's own and claim no RFC type code.  The head of size n is signed with leaf n and only with
 * it: the history is append-only, so that head never changes and two signatures of one size are byte-identical.  ONE SEED SERVES ONE
 * HISTORY: a registrar who starts another log under the same seed reuses one-time keys and makes its signatures forgeable.
 * Public key (KOSK_HEADSIG_PUB_BYTES): LE32(height) || I[16] || T[1][32].  Signature (kosk_headsig_sig_bytes(height) = 1136 + 32 height):
 * LE32(height), LE32(q), LE32(0), LE32(0), C[32], z[34][32], path[height][32].
 * Host functions (no handle, no GPU): kosk_headsig_sig_bytes is 0 for a height outside 1..24.  kosk_headsig_statement writes the 56 signed
 * bytes "kosk-sighead-v1" || 00 || root || LE32(size) || LE32(kyber_k); -1: NULL, kyber_k outside 2..4, size < 0.  kosk_headsig_verify: 1
 * valid, 0 invalid (the header's height differs from the key's, q != size, q >= 2^height, a non-zero reserved word, or the walk does not end
 * in T[1]), -1: NULL, bad kyber_k, size < 0, a height outside 1..24 in pub.  kosk_headsig_public_from_seed builds the public key on one
 * thread (2^height x 8714 permutations): the CPU baseline and the tests' oracle; -1: NULL or a bad height.
 * The signer lives on the registrar's handle.  kosk_registry_signer_reserve(height 1..24, seed, id, pub) needs a reserved history (of any
 * size), builds all 2^height leaves and the tree in HBM (64 x 2^height bytes) in launches of at most 65536 leaves, and returns the public
 * key; height 0 frees.  The same (height, id) over a standing tree restores the seed and builds nothing if the root matches: the call
 * recomputes leaf 0 from the seed and compares it with the tree's, which decides the same thing (the root is a function of the leaves);
 * the resident seed is replaced only after that match.  Freeing or re-reserving the history or the registry frees the signer.  kosk_registry_signer_level: the height (0: none) and
 * whether the seed is there.  kosk_registry_history_sign_head(size < 0: current) signs the head of `size`; the root is read where the
 * history keeps it in HBM and is returned with the signature (root and size_out may be NULL).  -1 with a text that begins with the call's
 * name and nothing started: no registry / history / signer, "seed was wiped", size above the current size, "signer is exhausted"
 * (size >= 2^height).  seed, id, pub, sig and root may be host or device memory of any alignment.
 * kosk_headsig_verify_heads: ok[b] = 1 iff kosk_headsig_verify(pub, kyber_k of the handle, roots + 32 b, sizes[b], sigs_b) returns 1, for
 * any n >= 1 in launch groups of 16384 under the rules of the relying party's calls above: no registry needed, host or device arrays of any
 * alignment, peer data gives a verdict and never a refusal; a bad height in pub is a refusal.
 * Erasure: the seed is a secret entry of the inventory and long-lived like the slot of kosk_kem_key_set:
 * kosk_wipe_secrets and kosk_destroy zero it, KOSK_WIPE_CALL leaves it.  After a wipe signing is refused and the tree and public key
 * stay.  The tree, the staged signature and the verifier's staging are public entries. */
#define KOSK_HEADSIG_PUB_BYTES 52
#define KOSK_HEADSIG_ITEMS_PER_BLOCK 7 /* one-time keys per block of k_headsig_leaves / k_headsig_verify: launch edges for tests */
size_t kosk_headsig_sig_bytes(int height);
int kosk_headsig_statement(int kyber_k, const uint8_t root[32], int size, uint8_t out[56]);
int kosk_headsig_verify(const uint8_t pub[52], int kyber_k, const uint8_t root[32], int size, const uint8_t *sig);
int kosk_headsig_public_from_seed(int height, const uint8_t seed[32], const uint8_t id[16], uint8_t pub[52]);
int kosk_registry_signer_reserve(kosk_ctx *ctx, int height, const uint8_t seed[32], const uint8_t id[16], uint8_t pub[52]);
int kosk_registry_signer_level(kosk_ctx *ctx, int *height, int *has_seed);
int kosk_registry_history_sign_head(kosk_ctx *ctx, int size, uint8_t *sig, uint8_t root[32], int *size_out);
int kosk_headsig_verify_heads(kosk_ctx *ctx, int n, const uint8_t pub[52], const uint8_t *roots, const int32_t *sizes, const uint8_t *sigs, uint8_t *ok);

/* crypto_kem_keypair_derand / crypto_kem_keypair (kyber/kem.c:25-57) for n >= 1 items, byte for byte: ordinary Kyber key pairs with an
 * independent z, on the KEM workspace alone (no prover workspace, no max_batch limit).  coins: n x 64 bytes, d || z per item; NULL: one
 * 64-byte draw per item, in item order, on the caller's thread, through the randombytes callback / OS entropy (kem.c:53-54).  pk / sk:
 * n records of kosk_pk_bytes / kosk_sk_bytes, sk = tobytes(NTT(s)) || pk || SHA3-256(pk) || z; host or device memory like every KEM
 * buffer.  The call does not touch the prover's and verifier's resident state (kosk_kem_enc_verified after it behaves as before it).
 * No branch and no address depends on d, the noise seed, s, e or z (only gen_matrix's rejection sampling, on the public rho, branches
 * on data); z is copied, never hashed.  The secret scratch (d || z, the noise seed, s, e, the sk records) stays in the handle's HBM
 * workspace until it is erased: kosk_wipe_secrets, KOSK_WIPE_CALL or kosk_destroy.  -1 with a text and nothing started
 * for n < 1 or a NULL pk / sk; -1 ("block limit", no results, device outputs untouched) if gen_matrix reached its block limit. */
int kosk_kem_keypair_batch(kosk_ctx *ctx, int n, const uint8_t *coins, uint8_t *pk, uint8_t *sk);
/* The input checks of FIPS 203 for n >= 1 records, host or device memory; flags: n bytes, host or device memory, flags[b] about
 * record b alone, 0 = passes.  Read-only: kosk_kem_enc_batch / kosk_kem_dec_batch keep folding fields >= q and trusting the stored
 * H(pk), whatever these calls say.  The test over s-hat is sign-mask arithmetic and an OR-reduction. */
#define KOSK_KEYCHK_HASH     1   /* SHA3-256(pk inside sk) != stored H(pk)          FIPS 203 7.3 */
#define KOSK_KEYCHK_PK_RANGE 2   /* a 12-bit field of t-hat is >= q                 FIPS 203 7.2 */
#define KOSK_KEYCHK_S_RANGE  4   /* a 12-bit field of s-hat is >= q                 (not in the standard; reported separately) */
int kosk_kem_check_pk(kosk_ctx *ctx, int n, const uint8_t *pk, uint8_t *flags);   /* 0 or KOSK_KEYCHK_PK_RANGE */
int kosk_kem_check_sk(kosk_ctx *ctx, int n, const uint8_t *sk, uint8_t *flags);   /* OR of the three; 0 = passes */

/* ---- Proofs for Kyber keys that already exist.  sk: n consecutive records of kosk_sk_bytes,
 * NTT(s) bytes || pk || H(pk) || z, from this library or any other Kyber implementation; host or device memory.  H(pk) and z are not read.
 * The witness is recovered on the device: s = NTT^-1(s-hat), e = NTT^-1(t-hat - A o s-hat) with t-hat and A from the pk INSIDE the record.
 * 12-bit fields >= q in s-hat and in that pk are folded mod q, as polyvec_frombytes and the KEM calls do (a proof over a pk with such a
 * field is still refused by the strict-encoding verifier).  ok[b] (host memory) = 1 iff every coefficient of s and e lies in
 * [-eta1, eta1] (eta1 = 3 for kyber_k 2, else 2), the range the proof is about: true for every honestly generated key, false for a
 * record whose halves do not belong together or that was tampered with.  Where ok[b] = 0 the witness written for b is all zero.
 * No branch and no address of the recovery depends on s-hat, s, e or the verdict.  The copy of the sk records, s and e stay in the
 * handle's HBM workspace until they are erased: kosk_wipe_secrets, KOSK_WIPE_CALL or kosk_destroy.
 * All five calls return -1 with a kosk_last_error text and start nothing for n out of range, a NULL sk / ok / pi or a stride below
 * one tape / seed, and -1 ("block limit", no results) if gen_matrix reached its block limit; else 0, and ok[] says which keys were proven.
 * They run unmerged on the handle's own stream(s): on a member of a cohort (combine >= 2) and with streams > 1 the staging calls and
 * kosk_witness_from_sk behave as kosk_stage_prover_inputs does (the sub-batches of kosk_prove_resident, on the handle's own view /
 * lanes), the host-buffer forms as kosk_verifiable_keygen_batch does without combining (chunks dealt to the handle's lanes). */
/* kernel level: n <= max_batch; se_out (host memory, may be NULL): n x 2 K x 256 int16, s then e per key; leaves A, t, s, e and the pk
 * bytes resident exactly as kosk_stage_prover_keys does */
int kosk_witness_from_sk(kosk_ctx *ctx, int n, const uint8_t *sk, int16_t *se_out, uint8_t *ok);
/* The counterpart of kosk_stage_prover_inputs[_seeded] for existing keys, n <= max_batch; then kosk_prove_resident and
 * kosk_fetch_proofs[_compact|_dense].  tapes: the format of every other call (kosk_tape_bytes per proof, host or device memory, a device buffer
 * read in place under the same alignment rule); the first 64 bytes of a tape, the key seed of a verifiable key generation, are NOT
 * read -- so on the sk that kosk_verifiable_keygen_batch(tape) returned, the proof is the one that call returned, byte for byte.
 * tapes / seeds == NULL: the handle's entropy mode (kosk_set_entropy) -- the draws of prepare_randomness, prepare_range_proof and
 * prove in the reference's order without the key generation's 64-byte draw, or one 32-byte draw per proof.
 * The proof left in HBM at a position with ok[b] = 0 was made from the all-zero witness (it does not verify); the other positions
 * are unaffected.  Afterwards the pk bytes, A and t of these keys are resident as after a key generation:
 * kosk_verify_resident_pk(pk == NULL) and then kosk_kem_enc_verified work on them. */
int kosk_stage_prover_keys(kosk_ctx *ctx, int n, const uint8_t *sk, const uint8_t *tapes, size_t tape_stride, uint8_t *ok);
int kosk_stage_prover_keys_seeded(kosk_ctx *ctx, int n, const uint8_t *sk, const uint8_t *seeds, size_t seed_stride, uint8_t *ok);
/* host-buffer forms, any n >= 1, chunked by max_batch like kosk_verifiable_keygen_batch: pi receives n proof images, all zero where ok[b] = 0 */
int kosk_prove_keys_batch(kosk_ctx *ctx, int n, const uint8_t *sk, const uint8_t *tapes, size_t tape_stride, uint8_t *pi, uint8_t *ok);
int kosk_prove_keys_seeded_batch(kosk_ctx *ctx, int n, const uint8_t *sk, const uint8_t *seeds, size_t seed_stride, uint8_t *pi, uint8_t *ok);

/* ---- The offline bank (INTEGRATION.md 14 is the normative text; the reference's offline / online split, mlwe_prover.cpp:4-59 against
 * :81-).  prepare_randomness and prepare_range_proof need no key: their output -- the 2M sharings of f / NTT f and the
 * 2K(2 eta1 + 1) range sharings of a proof -- can be made ahead of time and wait in HBM, and a proof then costs only the part that depends
 * on the key.  With M = 71 + 2K, E = 2 eta1 + 1 and T = kosk_tape_bytes(k) = 64 + 32M + 302 (2M + 2KE + 3K + 4K eta1) a tape has three
 * SECTIONS: 0 the key seed [0, 64), 1 offline [64, O) with O = 64 + 32M + 302 (2M + 2KE), 2 online [O, T).
 * A bank ENTRY is the offline rows of one proof as the offline pass leaves them in the row matrix (whole rows, packed secrets included),
 * kosk_bank_entry_bytes(k) bytes of HBM.  The bank is a FIFO ring of `capacity` entries owned by the handle: kosk_bank_fill appends,
 * and proof b of a consuming call takes the b-th oldest entry, also across max_batch chunks.
 * THE CONTRACT of every consuming call: for entry e and proof b it returns byte for byte (ok[], zero images, return codes and resident
 * state included) what the non-banked call returns on the SPLICED tape: key seed || offline section of the tape e was filled from ||
 * online section of the tape given to the consuming call.  For seeds "the tape" is kosk_tape_from_seed(seed).  The same tape on both
 * sides gives the proof of the existing call on that tape.  ONE EXCEPTION in the resident state: a banked proof leaves no staged prover
 * inputs.  After kosk_verifiable_keygen_banked_batch, after kosk_prove_keys_banked_batch, and after the ONE kosk_prove_resident behind
 * kosk_stage_prover_keys_banked, kosk_prove_resident returns -1 ("no resident prover inputs") until a staging call has run: the handle
 * never held these proofs' offline sections as a tape, and the rows of a consumed entry serve one proof.  The proofs, pk bytes, A and t
 * stay resident as after the non-banked call.
 * EXACTLY ONCE: two proofs on one entry open s + r and s' + r with the same r and so leak s - s'.  An entry is consumed exactly once:
 * the kernel that copies it out zeroes it in the same pass, taken entries never come back whatever happens afterwards (a later HIP error
 * included), and a position with ok[b] = 0 consumes its entry like any other.
 * Randomness arguments of the four calls that take them: at most one of tapes / seeds non-NULL (both: -1).  tapes are in the full format
 * of every other call, tape_stride >= T, host or device memory; only the section the call consumes is read (fill: 1; prove: 2; key
 * generation: 0 and 2), and from host memory only that section crosses PCIe.  seeds follow the seeded calls.  Both NULL: the handle's
 * entropy mode -- KOSK_ENTROPY_TAPE the reference's draws for that section in its order (fill: M x 32 then (2M + 2KE) x 302; consume:
 * (3K + 4K eta1) x 302, the key generation form with its 64-byte draw in front), KOSK_ENTROPY_SEED one 32-byte draw per entry / proof.
 * Every refusal (-1 with a kosk_last_error text) consumes nothing and writes nothing: argument errors, n larger than the level ("bank is
 * empty" at level 0), a full bank.  The bank needs streams = 1; on a member of a cohort (combine >= 2) the calls run unmerged on the
 * member's own block, as kosk_prove_keys_batch does.  An armed handle (kosk_set_contexts) makes bound proofs as the non-banked calls do.
 * ERASURE: the bank is a secret buffer of the inventory.  kosk_wipe_secrets zeroes it and sets the level to 0;
 * the wipe at the end of a call under KOSK_WIPE_CALL leaves unconsumed entries alone (a long-lived secret, like the key slot of 8.2) and
 * clears everything else; kosk_destroy and kosk_bank_reserve(0) wipe before they free; kosk_secret_scan sees the bank. */
size_t kosk_bank_entry_bytes(int kyber_k);                                            /* 0 for a bad k */
int kosk_tape_section(int kyber_k, int section, size_t *offset, size_t *size);        /* -1: bad k, bad section, NULL pointer */
/* HBM for exactly `capacity` entries: the handle's own allocation, made here and nowhere else.  Again only while the bank is empty (the
 * old allocation is wiped and freed first); 0 wipes and frees.  -1: capacity < 0, a non-empty bank, streams > 1 */
int kosk_bank_reserve(kosk_ctx *ctx, int capacity);
int kosk_bank_level(const kosk_ctx *ctx, int *ready, int *capacity);
/* n >= 1 entries appended in order, chunked by max_batch: the offline pass, then k_bank_put.  ready + n > capacity: -1, nothing changes.
 * Staged prover inputs (kosk_stage_prover_*) do not survive a fill */
int kosk_bank_fill(kosk_ctx *ctx, int n, const uint8_t *tapes, size_t tape_stride, const uint8_t *seeds, size_t seed_stride);
/* kosk_stage_prover_keys on n <= max_batch bank entries; then kosk_prove_resident(n), ONCE, which runs the online part only, and
 * kosk_fetch_proofs*.  After kosk_wipe_secrets kosk_prove_resident fails as after any staging call */
int kosk_stage_prover_keys_banked(kosk_ctx *ctx, int n, const uint8_t *sk, const uint8_t *tapes, size_t tape_stride,
                                  const uint8_t *seeds, size_t seed_stride, uint8_t *ok);
/* kosk_prove_keys_batch on n >= 1 bank entries */
int kosk_prove_keys_banked_batch(kosk_ctx *ctx, int n, const uint8_t *sk, const uint8_t *tapes, size_t tape_stride,
                                 const uint8_t *seeds, size_t seed_stride, uint8_t *pi, uint8_t *ok);
/* kosk_verifiable_keygen_batch on n >= 1 bank entries: the key seed and the online section of the tapes are read */
int kosk_verifiable_keygen_banked_batch(kosk_ctx *ctx, int n, const uint8_t *tapes, size_t tape_stride,
                                        const uint8_t *seeds, size_t seed_stride, uint8_t *pk, uint8_t *sk, uint8_t *pi);
/* diagnostic (tools/bank_rate.py): on an EMPTY bank of >= n entries, n <= max_batch: `reps` launches each of k_bank_put and k_bank_take
 * on n slots, of the runtime's own two strided D2D copies of the same bytes, and of those copies plus its fill of the slots; milliseconds
 * per repetition between two events; bytes = n x kosk_bank_entry_bytes.  The offline rows of the row matrix are overwritten */
int kosk_bank_timing(kosk_ctx *ctx, int n, int reps, double *put_ms, double *take_ms, double *copy_ms, double *copy_fill_ms, size_t *bytes);

/* Which kernel / copy paths ran on this handle since it was created (the tests of the fallbacks and of the Fiat-Shamir mode assert on
 * these).  ids: 0 commitment hash with LDS-DMA staging, 1 without (a layout the staged kernel cannot take: unaligned rows),
 * 2 shared-table products on k_table_gemm / k_table_gemm_p (every mod-q product), 3 retired, always 0 (the generic limb GEMM, which no call
 * could reach; the id keeps its number), 4 proof images copied straight between HBM and page-locked caller memory (kosk_host_alloc or locked by the
 * caller), 5 through the pinned staging buffer (pageable caller memory), 6 hipGraph segment replays (KOSK_GRAPHS=1), 7 commitment rounds
 * whose digest table was copied to the host (host Fiat-Shamir mode), 8 small copies between HBM and the library's own page-locked buffers
 * made by a copy kernel, 9 Fiat-Shamir rounds hashed on the device (k_fs_chain), 10 on the host, 11 launches of k_tape_expand (seeded
 * proving: tapes expanded from seeds in HBM), 12 kem_enc / 13 kem_dec: launch groups (up to 16384 items, three or four launches each) of the KEM calls,
 * 14 refills of the dense wire format (k_dense_setup + k_dense_fill, one per staged chunk or kosk_dense_fill_device sub-batch),
 * 15 kem_keypair / 16 kem_check: launch groups of kosk_kem_keypair_batch and of kosk_kem_check_pk / kosk_kem_check_sk,
 * 17 launches of k_keyseed (kosk-keyseed-v1: seeds derived from the sk records in HBM),
 * 18 launches of k_wipe (kosk_wipe_secrets, the wipe at the end of a call under KOSK_WIPE_CALL, kosk_wipe_device),
 * 19 launches of k_kem_key_setup (one per kosk_kem_key_set), 20 kem_enc_key / 21 kem_dec_key: launch groups of kosk_kem_enc_key /
 * kosk_kem_dec_key (ids 12 / 13 do not move for them),
 * 22 launches of k_dense_check (the codeword check: one per chunk of kosk_transcode_batch to dense or kosk_dense_check_device sub-batch),
 * 23 refills of kosk-dense-v2 (k_dense2_setup + k_dense2_fill) / 24 launches of k_dense2_check, counted like 14 / 22, which do not move
 * for v2 work,
 * 25 launches of k_bank_put (one per chunk of kosk_bank_fill) / 26 launches of k_bank_take (one per chunk of a call that consumes bank
 * entries); the diagnostic kosk_bank_timing moves both by reps + 1,
 * 27 launches of k_registry_admit (one per launch group of kosk_registry_admit / kosk_registry_admit_verified), 28 kem_enc_slots: launch
 * groups of kosk_kem_enc_slots (ids 12 / 20 do not move for it); kosk_registry_evict runs k_wipe (id 18),
 * 29 launches of k_registry_index (one per rebuild of the fingerprint index: the first lookup after a mutation of the registry),
 * 30 launches of k_registry_find (one per launch group of kosk_registry_find, kosk_registry_enrol* and kosk_kem_enc_peers),
 * 31 kem_enc_peers: launch groups of kosk_kem_enc_peers (ids 12 / 20 / 28 do not move for it),
 * 32 launches of k_registry_tree (one per tier of a rebuild) / 33 leaf subtrees hashed by those launches,
 * 34 launches of k_registry_path (one per launch group of kosk_registry_prove_slots / kosk_registry_prove_peers),
 * 35 launches of the sort kernels k_regsort_keys / k_regsort_tile / k_regsort_step (a rebuild of the sorted tree, or kosk_regsort_order_device),
 * 36 launches of k_regsort_tree (one per tier of a rebuild of the sorted tree; ids 27..34 do not move for any call of that section),
 * 37 launches of k_regsort_prove (one per launch group of kosk_registry_prove_absent),
 * 38 launches of k_reghist_append (one per tier of an append to the registry history) / 39 leaf groups hashed by those launches (the
 * tier-0 blocks: ((s + c - 1) >> 10) - (s >> 10) + 1 for c events appended at size s),
 * 40 launches of k_reghist_frontier (the ragged nodes and the root of one size; a second call at the same size launches nothing),
 * 41 launches of k_reghist_prove (one per launch group of kosk_registry_history_prove_events / _prove_consistency; ids 27..37 do not move
 * for kosk_registry_history_head, _read or the proving calls),
 * 42 launches of k_monitor_keys (one per segment of kosk_monitor_feed),
 * 43 launches of k_monitor_apply (two per segment: check, then commit),
 * 44 launches of k_monitor_leaves (one per tier-0 append of the monitor's history),
 * 45 launches of k_monitor_check (one per checkpoint event fed); the kernels the monitor reuses count in their own ids (32, 33, 35, 36,
 * 38..40) on the monitor's handle: the slot tree's tiers and subtrees, the sort network of every segment and of every rebuild of the
 * sorted tree, the history's upper tiers and leaf groups, the frontier; ids 42..45 do not move for kosk_monitor_head, _roots, _read or
 * _level,
 * 46 launches of k_regtree_check (one per launch group of kosk_regtree_check_paths, and one per launch group of kosk_kem_enc_proven),
 * 47 launches of k_regsort_check (one per launch group of kosk_regsort_check_proofs),
 * 48 kem_enc_proven: encapsulation launches of kosk_kem_enc_proven, one per launch group (ids 0..45 do not move for any call of that
 * section: its encapsulation is counted here, not on id 12),
 * 49 launches of k_headsig_leaves (ceil(2^height / 65536) per build of kosk_registry_signer_reserve; one for a reserve that only restores
 * the seed over a standing tree),
 * 50 launches of k_headsig_tree (one per tier of a build: ceil(height / 10)),
 * 51 launches of k_headsig_sign (one per kosk_registry_history_sign_head; the frontier it needs counts on id 40),
 * 52 launches of k_headsig_verify (one per launch group of kosk_headsig_verify_heads); ids 0..48 do not move for any call of that section
 * except id 40. */
int kosk_path_count(const kosk_ctx *ctx, int id, long *count);
/* host worker threads per sub-context (kosk_options::host_threads; else <= 8, <= CPUs of the process / streams; all created by kosk_create) */
int kosk_host_threads(const kosk_ctx *ctx);

/* wall seconds of the phases of the last prove / verify on this context (16 values: host_pre, gpu_commit,
 * fs_alpha, gpu_relation, fs_open, gpu_assemble, d2h, then the host time spent issuing the prover's three
 * segments, and the verifier's issue1, wait1, fs_alpha, issue2, wait2, fs_open) */
int kosk_phase_seconds(const kosk_ctx *ctx, double *out, int n);

/* HIP-event timing of the library's own launches on its stream.  ids: 0 prover Tcomm hash, 1 prover view
 * hash, 2 expansion GEMM #1, 3 expansion GEMM #2, 4 beta/gamma lincomb, 5 NTT(f), 6 wire image,
 * 7/8 verifier Tcomm/view hash, 9 interpolation operators, 10 interpolation GEMM, 11 verifier expansion,
 * 12 reconstruction GEMM, 13 verifier lincomb.  Reading returns the sum over launches since enable.
 * on = 1: only the view-commitment hashes (ids 1 and 8), which are plain launches; everything else keeps
 * running as captured hipGraph segments (the production path).  on = 2: every id, with plain stream launches
 * instead of graphs (diagnostic: changes the launch overhead being measured).  on = 0: off. */
int kosk_profile_enable(kosk_ctx *ctx, int on);
int kosk_profile_read(const kosk_ctx *ctx, int id, double *total_ms, long *launches);
/* the same plus the proofs those launches served: a merged run of a cohort (call combining, below) serves several callers'
 * batches per launch, and its launches are timed on the handle that led the run */
int kosk_profile_read_units(const kosk_ctx *ctx, int id, double *total_ms, long *launches, long *proofs);

/* ---- Call combining (no reference counterpart: the reference is one call, one proof, one thread -- kosk.hpp:18-24).
 * With kosk_options::combine = C (2..16, needs streams = 1), handles created with equal (device, kyber_k,
 * max_batch) are grouped into cohorts of C that share one workspace, and the resident calls kosk_verifiable_keygen_resident /
 * kosk_verify_resident_pk that neighbouring members of a cohort make at about the same time -- each from its own thread --
 * are served by ONE pipeline run over all their proofs: every launch then covers 2..C callers' batches, which is what the
 * chip-filling kernels need (a 46-proof launch leaves the commitment hash at one and a bit rounds of waves per SIMD).  Per
 * call nothing changes: same arguments, same results byte for byte, each caller gets its own pk / sk / verify bits / fail
 * masks / resident proofs (kosk_resident_proofs, kosk_resident_digests point at the member's own block).  A member's call
 * waits at most combine_wait_us (default 5000) for the other members, and only for those that are inside a call or left
 * one less than combine_idle_us (default 1000) ago: a lone caller is never delayed, callers that loop fall into step after
 * one or two calls (a request whose kind is in the minority of its window is held back once, so that callers alternating
 * keygen / verify in opposite phase meet).  The callers of a merged run sleep while it executes and are woken shortly before its
 * end (they then spin at most combine_prewake_us, default 400, for the return).  Calls that draw whole tapes through
 * the callback (tapes == NULL in the default entropy mode) and every other entry point run unmerged on the member's own block; seeded
 * calls merge like calls with tapes (their seeds, given or drawn on the caller's own thread, are expanded by the run).  A member's round hook
 * (kosk_set_round_hook) fires from a merged run as well, with that member's block of the table, ON THE THREAD OF THE RUN'S LEADER while
 * the member's own caller sleeps inside its call: a hook that relies on thread-local state (a current device, a stream context, a
 * thread-affine communicator) or that blocks must opt out with kosk_options::hooks_unmerged = 1, which keeps the calls of a handle
 * with a hook out of merged runs.  A cohort is formed by handles whose options agree (combine, strict_encoding, fs_mode,
 * host_threads, blocking_sync).  All handles of a cohort must be destroyed before the process ends (the last one frees the workspace).
 * kosk_combine_stats: resident calls of THIS handle that went through the combiner, and the sum over those calls of the
 * members their run served (members / calls = mean callers per launch; both 0 for a handle outside a cohort). */
int kosk_combine_stats(const kosk_ctx *ctx, long *calls, long *members);

/* hipEvent pair on the ctx stream around caller-issued kernel-level calls (micro-benchmarks) */
int kosk_stream_timer_start(kosk_ctx *ctx);
int kosk_stream_timer_stop(kosk_ctx *ctx, double *ms);

/* ---- kernel-level entry points on DEVICE pointers (stream 0 of the ctx) ----
 * Used by the parity tests and by bench.py's roofline leg.  Every stream of the library is a NON-BLOCKING HIP stream: it is not
 * ordered against the legacy null stream (nor against any other stream of the caller).  Device buffers handed to these entry
 * points -- and device tapes / keys handed to the resident calls -- must be complete before the call (synchronise the stream
 * that produced them), and kosk_device_synchronize() must have returned before another stream reads the outputs. */

/* sha3_256(h, in, inlen) for n equal-length messages        kyber/fips202.c:745-754
 * message-major layout: message i at in + i*in_stride; digest i at out + 32*i */
int kosk_sha3_256_batch(kosk_ctx *ctx, const uint8_t *d_in, size_t in_stride, size_t inlen, uint8_t *d_out, int n);
/* the same function computed by the lane-pair ("warp-cooperative") sponge: one Keccak state spread over two adjacent lanes of a
 * wave, 64-bit rotations exchanged by DPP, 32 messages per wave (csrc/kosk_keccak_split_dev.hpp; BASELINE.json north_star names
 * this layout; the pipeline's hashes use one lane per state, which is faster at its wave counts -- DESIGN.md 8) */
int kosk_sha3_256_batch_pair(kosk_ctx *ctx, const uint8_t *d_in, size_t in_stride, size_t inlen, uint8_t *d_out, int n);
/* sha3_256 of n LONG messages, one WAVE per message: one Keccak state spread over the 64 lanes
 * of a wave, a 32-bit word of the bit-interleaved state per lane, theta / pi / chi exchanged by DPP and ds_bpermute
 * (csrc/kosk_keccak_wave_dev.hpp) --
 * the layout for a strictly sequential chain: ~2 us per permutation where the one-state-per-lane sponge needs ~9 us when its wave
 * runs alone.  d_in and in_stride must be multiples of 8.        kyber/fips202.c:745-754 */
int kosk_sha3_256_batch_wave(kosk_ctx *ctx, const uint8_t *d_in, size_t in_stride, size_t inlen, uint8_t *d_out, int n);
/* kosk_fs_alpha / kosk_fs_opened (below) on n digest tables [1454][32] in HBM, table_stride bytes apart (multiples of 8): what a
 * handle in device Fiat-Shamir mode runs between its commitment kernels and their consumers (mlwe_prover.cpp:130-153, :445-474).
 * d_alpha: n x 80 u16 (70 + 2K derived, zeros behind); d_h1 / d_ch: optional n x 32 bytes, the tables' sha3_256.
 * d_sel: n rows of sel_stride u16 -- I in [0, 150), at 160 + w the number of unopened parties below 64 w (w = 0..23), at 192 the
 * opened parties ascending and at 352 their positions in I; d_rest: n rows of sel_stride u16, the ascending complement (1304). */
int kosk_fs_alpha_device(kosk_ctx *ctx, const uint8_t *d_tables, size_t table_stride, int n, uint16_t *d_alpha, uint8_t *d_h1);
int kosk_fs_opened_device(kosk_ctx *ctx, const uint8_t *d_tables, size_t table_stride, int n, uint16_t *d_sel, uint16_t *d_rest, int sel_stride, uint8_t *d_ch);
/* shake256(out, outlen, in, inlen)                           kyber/fips202.c:723-734 */
int kosk_shake256_batch(kosk_ctx *ctx, const uint8_t *d_in, size_t in_stride, size_t inlen,
                        uint8_t *d_out, size_t outlen, int n);
/* kosk-seedtape-v1 (above) for n seeds at once: seeds host or device memory (seed_stride >= KOSK_SEED_BYTES), tapes DEVICE memory,
 * tape b at d_tapes + b * tape_stride (base and tape_stride multiples of 8, tape_stride >= kosk_tape_bytes); nothing outside the
 * kosk_tape_bytes() bytes of each tape is written.  n <= max_batch.  Synchronised on return. */
int kosk_tape_expand_device(kosk_ctx *ctx, int n, const uint8_t *seeds, size_t seed_stride, uint8_t *d_tapes, size_t tape_stride);
/* The view-commitment kernel on its native column layout: lane l hashes
 * [prefix32(l)] || rows[r][l], r < words, rows being u16 arrays `row_stride`
 * elements apart (mlwe_prover.cpp:116-127 when with_prefix == 0, :397-444 when 1).
 * words must equal the Tcomm / view word count of kyber_k. */
int kosk_commit_hash_lanes(kosk_ctx *ctx, const uint16_t *d_rows, size_t row_stride, int n_lanes,
                           const uint8_t *d_prefix, int with_prefix, uint8_t *d_out);
/* poly_ntt(r) on n polynomials of 256 int16                  kyber/poly.c:261-265 (ntt.c:80-95 + Barrett) */
int kosk_ntt256_batch(kosk_ctx *ctx, const int16_t *d_in, int16_t *d_out, int n);
/* share values of all 1454 parties from the 407 values at points 0..406
 * (recompute_share_secrets_ddeg, ss.cpp:76-99): in  n x 407 u16, out n x 1454 u16.
 * Input values >= q are folded mod q where they enter a product; shares 0..127 are the row's own values at points 256..383,
 * copied as given: a value >= q there comes back unreduced (every computed share, 128..1453, is canonical). */
int kosk_lagrange_expand(kosk_ctx *ctx, const uint16_t *d_y407, uint16_t *d_shares, int n);
/* recon_secrets_ddeg / recon_secrets_2ddeg (ss.cpp:37-73): in n x 1454 u16, out n x 256 u16 */
int kosk_recon_secrets(kosk_ctx *ctx, const uint16_t *d_shares, uint16_t *d_secrets, int n, int two_d);
int kosk_device_synchronize(kosk_ctx *ctx);
/* number of sub-batches a handle keeps in flight on separate HIP streams (kosk_options::streams, default 1) */
int kosk_streams(const kosk_ctx *ctx);
/* device pointer / stride of the resident proof images of sub-batch 0, for callers chaining work in HBM
 * (with streams = 1 this is the whole batch) */
int kosk_resident_proofs(kosk_ctx *ctx, void **d_proofs, size_t *stride);
/* The per-party commitment digests in HBM: round 0 = Tcomm[1454][32] of every proof of the last batch
 * (mlwe_prover.cpp:116-127, the input of sha3_256(Tcomm[0..N)) at :130-135), round 1 = the view commitments
 * (:397-444, input of :445-449); `stride` = bytes per proof (1454 * 32).  This is what a multi-GPU job all-gathers
 * (RCCL) after each commitment round (BASELINE.json configs[3]).  Needs streams = 1. */
int kosk_resident_digests(kosk_ctx *ctx, int round, void **d_digests, size_t *stride);
/* Called on the calling thread -- for a call served by a merged run of a cohort (call combining): on the thread of the caller that
 * leads the run, while this handle's own caller sleeps inside its call -- as soon as a round's table is complete in HBM (role 0
 * prover / 1 verifier; round as above; bytes = n * 1454 * 32; d_digests = this handle's own block); the context's stream may
 * already be running the kernels of the next segment, none of which writes the tables.  The place to start that all-gather so that it overlaps the host's Fiat-Shamir hashing.
 * fn == NULL removes the hook. */
typedef void (*kosk_round_fn)(void *user, int role, int round, const void *d_digests, size_t bytes);
int kosk_set_round_hook(kosk_ctx *ctx, kosk_round_fn fn, void *user);

/* ---- host-only pieces of the path (no device needed) ------------------------ */

/* void kyber_keygen(kyber_keypair *keypair, mlwe_inst *raw_key)      kosk.hpp:18-19, kosk.cpp:4-70
 * seed64 = the 64 bytes the reference draws with randombytes (kosk.cpp:12).
 * Raw key (mlwe_inst, mlwe_prover.hpp:34-37): A [K][K][256] NTT domain in [0,q),
 * s,e [K][256] small signed, t [K][256] NTT domain centred.  Any of A/s/e/t may be NULL. */
int kosk_keygen(int kyber_k, const uint8_t seed64[64], uint8_t *pk, uint8_t *sk,
                int16_t *A, int16_t *s, int16_t *e, int16_t *t);
/* alpha challenge from the 1454 Tcomm digests (mlwe_prover.cpp:130-142); alpha has 70+2K entries */
int kosk_fs_alpha(int kyber_k, const uint8_t *tcomm_all, uint16_t *alpha);
/* opened set I[150] and its ascending complement rest[1304] from the 1454 view digests
 * (mlwe_prover.cpp:445-490) */
int kosk_fs_opened(const uint8_t *digests_all, uint16_t *I, uint16_t *rest);
/* host sha3_256 / shake256 used by the two functions above (kyber/fips202.c:745-754, :723-734) */
void kosk_host_sha3_256(uint8_t out[32], const uint8_t *in, size_t inlen);
void kosk_host_shake256(uint8_t *out, size_t outlen, const uint8_t *in, size_t inlen);
/* sha3_256 of `count` equal-length messages with the SIMD multi-buffer code of the Fiat-Shamir rounds;
 * returns the SIMD width used (8 AVX-512, 4 AVX2, 1 scalar) */
int kosk_host_sha3_256_multi(uint8_t *out, const uint8_t *in, size_t in_stride, size_t inlen, int count, int nthreads);
/* Lagrange coefficient tables the reference reads through utils/precomputed_kyber.h:10-13:
 * which = 0: share_coeff_ddeg [1303][407], 1: recon_coeff_ddeg [256][407], 2: recon_coeff_2ddeg [256][813] */
int kosk_lagrange_table(int which, uint16_t *out);

/* ---- context-bound proofs, format kosk-bind-v1 (no reference counterpart) ----
 * For Kyber parameter K, public key bytes pk and a caller's 32-byte context (a hash of an identity, nonce or message):
 *   B  = SHA3-256("kosk-bind-v1" || 00 00 00 00 || LE32(K) || SHA3-256(pk) || context)            84 bytes
 *   h1 = SHA3-256(Tcomm[0..1454) || B)        ch = SHA3-256(view_digest[0..1454) || B)
 * and everything else as in the reference: alpha from h1, I from ch, the proof image and the tape consumption.  A bound proof verifies
 * only under the pk and the context it was made for. */
/* B on the host (no handle) */
int kosk_bind_value(int kyber_k, const uint8_t *pk, const uint8_t context[32], uint8_t out[32]);
/* B for n proofs on the device (k_bind_values): pk = n records of kosk_pk_bytes, contexts = n records context_stride >= 32 apart, each
 * host or device memory; d_out = n x 32 bytes of DEVICE memory, 8-byte aligned; nothing outside them is written.  Synchronised on return. */
int kosk_bind_device(kosk_ctx *ctx, int n, const uint8_t *pk, const uint8_t *contexts, size_t context_stride, uint8_t *d_out);
/* kosk_fs_alpha / kosk_fs_opened with the binding value hashed behind the table */
int kosk_fs_alpha_bound(int kyber_k, const uint8_t *tcomm_all, const uint8_t bind[32], uint16_t *alpha);
int kosk_fs_opened_bound(const uint8_t *digests_all, const uint8_t bind[32], uint16_t *I, uint16_t *rest);
/* kosk_fs_alpha_device / kosk_fs_opened_device with d_bind = n x 32 bytes (8-byte aligned), proof b's table followed by d_bind[b] */
int kosk_fs_alpha_bound_device(kosk_ctx *ctx, const uint8_t *d_tables, size_t table_stride, int n, const uint8_t *d_bind, uint16_t *d_alpha, uint8_t *d_h1);
int kosk_fs_opened_bound_device(kosk_ctx *ctx, const uint8_t *d_tables, size_t table_stride, int n, const uint8_t *d_bind,
                                uint16_t *d_sel, uint16_t *d_rest, int sel_stride, uint8_t *d_ch);
/* ARM the handle with n contexts (host or device memory, context_stride >= 32 apart; the handle keeps its own copy).  From then on every
 * first-level entry point that makes or checks proofs on this handle makes or checks BOUND proofs, position b of a call (of the whole call,
 * when it is chunked) under context b: kosk_verifiable_keygen_* (tape, seeded, compact, dense, resident), kosk_prove_resident after
 * kosk_stage_prover_inputs* / kosk_stage_prover_keys*, kosk_prove_keys_*, kosk_verify_batch[_compact|_dense], kosk_verify_resident after
 * kosk_stage_verifier_inputs*, kosk_verify_resident_pk.  Refused with -1 and a text, nothing started: a call of more proofs than armed
 * contexts; kosk_verify_inst / kosk_prove_prepared (no pk bytes exist there); context_stride < 32.  kosk_set_contexts(ctx, 0, NULL, 0)
 * disarms; a handle never armed, or disarmed, behaves exactly as before.  A cohort member that is armed keeps its calls out of merged
 * runs.  Not to be called while another thread is inside a call on this handle. */
int kosk_set_contexts(kosk_ctx *ctx, int n, const uint8_t *contexts, size_t context_stride);

/* ---- TESTS ONLY: the prover at a chosen opened list ----
 * While n lists are set (cand: host memory, n x 150 entries, each < 1454; the handle keeps its own copies), Fiat-Shamir round 2 of this
 * handle's PROVER takes cand[b][i] for proof b of a call (of the whole call, when it is chunked) in place of the candidates BE16 % 1454
 * it reads from the PRF output.  The probing (duplicates are allowed: they are what reaches it), the complement and the derived tables
 * are the code the honest path runs, in both Fiat-Shamir modes; ch and the view digests stay the honest ones, so the proof fails the
 * verifier's last check, I' == I, and no other.  kosk_fs_opened_device / kosk_fs_opened_bound_device obey it for tables b < n.  The
 * verifier never does.  -1 with a text, and the lists that were set stay: an entry >= 1454; n < 1 or n > KOSK_FORCE_MAX_LISTS; a handle
 * that replays captured graphs (KOSK_GRAPHS=1); a cohort member (combine).  A proving call of more proofs than lists fails with -1 (a
 * chunked call: at the first chunk that reaches behind the lists).  cand == NULL clears; kosk_destroy clears too.  Not to be called
 * while another thread is inside a call on this handle. */
#define KOSK_FORCE_MAX_LISTS 4096
int kosk_force_opened_candidates(kosk_ctx *ctx, int n, const uint16_t *cand);
/* the host's round-2 function behind the PRF on one candidate list, no handle: sel[0..150) = I, sel[160..184) the window boundaries,
 * sel[192..342) the opened parties ascending, sel[352..502) their positions in I; rest[0..1304) the ascending complement.  Nothing else
 * of the two rows is written.  -1: a NULL pointer, an entry >= 1454, sel_stride < 1304 (a row of the opened-list tables) */
int kosk_opened_tables(const uint16_t cand[150], uint16_t *sel, uint16_t *rest, int sel_stride);

/* ---- proof randomness derived from the key, format kosk-keyseed-v1 (no reference counterpart) ----
 *   seed = SHAKE256("kosk-keyseed-v1" || 00 || LE32(K) || LE32(flags) || context[32] || salt[32] || sk[kosk_sk_bytes(K)])[0 : 32]
 *   flags bit 0: the proof is context-bound (a context is given / the handle is armed), bit 1: a salt is given; a field whose bit is
 *   clear is 32 zero bytes.  tape = kosk-seedtape-v1(seed).
 * The sk record is hashed as it stands.  The proof is byte for byte what kosk_prove_keys_seeded_batch(sk, seed) returns on the same
 * handle state; the seed is as secret as the key, is made in HBM by k_keyseed and never reaches the host in the handle calls.
 * Without salts the call is a pure function of (sk, K, armed context): the same inputs give the same proof, any other input an
 * unrelated tape.  With salts (fresh random bytes per proof) it is the hedged form. */
/* the seed on the host (no handle); context == NULL: unbound, salt == NULL: none.  -1 for kyber_k outside 2..4, a NULL sk or seed */
int kosk_keyseed_value(int kyber_k, const uint8_t *sk, const uint8_t *context, const uint8_t *salt, uint8_t seed[32]);
/* kernel level (k_keyseed), any n >= 1: sk = n records of kosk_sk_bytes; contexts (NULL: unbound) and salts (NULL: none) n records
 * context_stride / salt_stride >= 32 apart; each host or device memory.  d_seeds = n x 32 bytes of DEVICE memory, 8-byte aligned
 * (else -1 and a text); nothing outside them is written.  Synchronised on return. */
int kosk_keyseed_device(kosk_ctx *ctx, int n, const uint8_t *sk, const uint8_t *contexts, size_t context_stride,
                        const uint8_t *salts, size_t salt_stride, uint8_t *d_seeds);
/* kosk_stage_prover_keys_seeded / kosk_prove_keys_seeded_batch with the seeds derived on the device: the context of position b is armed
 * context b of the whole call (also across max_batch chunks and streams > 1 sub-batches), flag 0 and a zero field on an unarmed handle.
 * salts == NULL: the deterministic form; else n records salt_stride >= 32 apart, host or device memory.  Everything else -- ok[], zero
 * images, return codes, the resident state, unmerged on a cohort member -- as the seeded calls above; more proofs
 * than armed contexts, or salt_stride < 32: -1 and a text, nothing started. */
int kosk_stage_prover_keys_derived(kosk_ctx *ctx, int n, const uint8_t *sk, const uint8_t *salts, size_t salt_stride, uint8_t *ok);
int kosk_prove_keys_derived_batch(kosk_ctx *ctx, int n, const uint8_t *sk, const uint8_t *salts, size_t salt_stride, uint8_t *pi, uint8_t *ok);

#ifdef __cplusplus
}
#endif
#endif /* KOSK_MI355X_H */
