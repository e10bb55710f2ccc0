// Host-side pieces of the product path: the Fiat-Shamir hashing that stays on
// the CPU by design (BASELINE.json north_star), Kyber key generation
// (host for now), Lagrange table generation, and a small
// thread pool.  None of this touches oracle/.
#pragma once
#include <cstddef>
#include <cstdint>
#include <functional>
#include <vector>

#include "kosk_params.hpp"

namespace kosk {

// fips202.c:745-774, :723-734, symmetric-shake.c:43-51
void sha3_256(uint8_t out[32], const uint8_t *in, size_t inlen);
void sha3_512(uint8_t out[64], const uint8_t *in, size_t inlen);
void shake128(uint8_t *out, size_t outlen, const uint8_t *in, size_t inlen);
void shake256(uint8_t *out, size_t outlen, const uint8_t *in, size_t inlen);
void shake256_prf(uint8_t *out, size_t outlen, const uint8_t key[32], uint8_t nonce);

// kosk.cpp:4-70.  A is [K][K][256] canonical, s/e are [K][256] small signed,
// t is [K][256] centred NTT-domain; pk/sk in Kyber wire format.
struct HostKey {
    int16_t A[MAXK * MAXK * 256];
    int16_t se[2 * MAXK * 256]; // s polys then e polys
    int16_t t[MAXK * 256];
};
void host_keygen(const Params &P, const uint8_t seed64[64], uint8_t *pk, uint8_t *sk, HostKey &key);
// kosk.cpp:94-110: decode pk into A (canonical) and t (12-bit values as stored)
void host_decode_pk(const Params &P, const uint8_t *pk, HostKey &key);

// mlwe_prover.cpp:130-142: alpha_j = BE16(SHAKE256(sha3_256(Tcomm) || 1)) % q
// bind (fs_alpha, fs_opened and their batch forms; nullptr: the reference's transcript): kosk-bind-v1, the 32-byte binding value follows the
// table in the hashed message -- a suffix of the multi-buffer hash's last block (46 528 = 342 x 136 + 16), no copy of the table
void fs_alpha(const Params &P, const uint8_t *tcomm_all /* [1454][32] */, uint16_t *alpha /* [J] */, const uint8_t *bind = nullptr);
// kosk-bind-v1: B = sha3_256("kosk-bind-v1" || 00 00 00 00 || LE32(K) || sha3_256(pk) || context); the host definition
// of what k_bind_values (kosk_fs_kernels.hip) computes on the device
void bind_value(const Params &P, const uint8_t *pk, const uint8_t context[32], uint8_t out[32]);
// kosk-keyseed-v1: seed = SHAKE256("kosk-keyseed-v1" || 00 || LE32(K) || LE32(flags) || context || salt || sk)[0:32], flags
// bit 0: context given, bit 1: salt given (a missing field is 32 zero bytes); the host definition of what k_keyseed computes on the device
void keyseed_value(const Params &P, const uint8_t *sk, const uint8_t *context, const uint8_t *salt, uint8_t seed[32]);
// mlwe_prover.cpp:445-474: opened list I (with the linear-probing de-dup) and its complement
void fs_opened(const uint8_t *digests_all /* [1454][32] */, uint16_t I[NOPEN], uint16_t rest[NREST], const uint8_t *bind = nullptr);

// Lagrange basis over n consecutive integer nodes a..a+n-1 evaluated at t
// (utils/precomputed_kyber.h:10-13; values by the call sites ss.cpp:26-27,:47,:66)
void lagrange_row(uint16_t *row, int n, int a, int t);
uint16_t gf_inv_host(uint16_t a);

// Persistent worker pool.  One per library context: several contexts (pipeline slots) run their
// Fiat-Shamir rounds concurrently, each on its own few threads.
class Pool;
Pool *pool_create();
void pool_destroy(Pool *);
// create the workers for jobs of up to `nthreads` threads now; returns the threads such a job will really run on (>= 1:
// thread creation may fail under a pid / thread limit, the pool then works with what it has)
int pool_reserve(Pool *, int nthreads);
// CPUs this process may run on (sched_getaffinity), the cap for every host thread count in the library
int host_cpu_count();
// run fn(i) for i in [0,n) on up to nthreads threads of `pool` (nullptr: a process-wide default pool)
void parallel_for(Pool *pool, int n, int nthreads, const std::function<void(int)> &fn);
inline void parallel_for(int n, int nthreads, const std::function<void(int)> &fn) { parallel_for(nullptr, n, nthreads, fn); }

// sha3_256 of `count` equal-length messages in[i] -> out + 32*i, `width` (4 or 8) at a time in SIMD
// lanes when the CPU has AVX2 / AVX-512F (runtime dispatch, scalar otherwise).  Used for the
// 46 528-byte Fiat-Shamir hashes (mlwe_prover.cpp:135, :449), which are sequential per proof.
void sha3_256_multi(uint8_t *out, const uint8_t *const *in, size_t len, int count);
int sha3_multi_width(); // 8 (AVX-512F), 4 (AVX2) or 1

// One proof's digest table [1454][32] on the verifier's host, put together from what the proof itself carries -- the digests of
// the 1304 unopened parties, ascending (fields Tcomm / comm of mpcith_proof, mlwe_verifier.cpp:36-38, :645-647) -- and the 150
// digests the verifier recomputed for the opened parties, in the order of the list I (:22-35, :585-632).  Memory-safe for a
// malformed I (out-of-range or repeated entries: the table is then garbage, and the proof is rejected for the list anyway).
void assemble_digest_table(uint8_t *table, const uint16_t *I, const uint8_t *unopened, const uint8_t *opened);

// batch forms of fs_alpha / fs_opened over n proofs whose digest tables are dig_stride bytes apart
// prep (optional): called for proof b on the worker that hashes it, before the hashing (the verifier assembles the table there)
void fs_alpha_batch(const Params &P, int n, const uint8_t *digs, size_t dig_stride, uint16_t *alpha, size_t alpha_stride, int nthreads, Pool *pool = nullptr,
                    const std::function<void(int)> *prep = nullptr, const uint8_t *bind = nullptr /* [n][32] */);
// windows: also write, behind each proof's list I (at I + SEL_WIN), the NWIN + 1 boundaries of the complement's aligned 64-party windows
// cand (tests, kosk_force_opened_candidates): proofs b < cand_n take cand[b][0..150), every entry < NPARTY, in place of the candidates
// BE16 % NPARTY of the PRF output; the table is hashed all the same
void fs_opened_batch(int n, const uint8_t *digs, size_t dig_stride, uint16_t *I, uint16_t *rest, size_t sel_stride, int nthreads, Pool *pool = nullptr,
                     bool windows = false, const std::function<void(int)> *prep = nullptr, const uint8_t *bind = nullptr /* [n][32] */,
                     const uint16_t *cand = nullptr /* [cand_n][NOPEN] */, int cand_n = 0);
// what lies behind the PRF in fs_opened / fs_opened_batch: the probing of 150 candidates (each < NPARTY) into the list I and its ascending
// complement, and the tables derived from them behind I (SEL_WIN, SEL_OSORT, SEL_OPOS of kosk_params.hpp; `Ib` is a row of >= SEL_OPOS + NOPEN entries)
void opened_from_candidates(const uint16_t cand[NOPEN], uint16_t I[NOPEN], uint16_t rest[NREST]);
void opened_derived_tables(uint16_t *Ib, const uint16_t rest[NREST]);

// OS entropy (kyber/randombytes.c:44-57, Linux branch)
void os_randombytes(uint8_t *out, size_t len);

// Seeded proving, format kosk-seedtape-v1 (no reference counterpart): the randomness tape of one 32-byte seed,
//   block_j = SHAKE256(seed || "kosk-seedtape-v1" || LE32(K) || LE32(j))[0:136],  tape = (block_0 || block_1 || ...)[0:tape_bytes]
// (the host definition of what k_tape_expand, kosk_tape_kernels.hip, computes on the device)
constexpr int SEED_BYTES = 32;
void tape_from_seed(const Params &P, const uint8_t seed[SEED_BYTES], uint8_t *tape);

} // namespace kosk
