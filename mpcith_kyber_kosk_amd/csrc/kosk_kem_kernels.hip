// Kyber KEM on gfx950: crypto_kem_enc_derand / crypto_kem_dec (kyber/kem.c:76-96, :140-169) for batches of items, bit-exact.
//
// Three launches per chunk of up to KEM_CHUNK items (plus one wave-sponge launch in a small chunk, below), all on the context's stream:
//   encapsulate   k_kem_hash    roles  H(pk) + G            one sponge per lane   (K^2 + 1) lanes per item
//                                      gen_matrix (A^T)
//                 k_kem_hash    roles  r, e1, e2            one sponge per lane   (2 K + 1) lanes per item
//                 k_kem_encrypt NTT(r), A^T o r-hat, t-hat o r-hat, inverse NTT, + e, compress, pack   one workgroup per item
//   decapsulate   k_kem_decrypt decompress, NTT(u), s-hat o u-hat, inverse NTT, tomsg, G(m' || h)     one workgroup per item
//                 k_kem_hash    roles  rkprf, gen_matrix, r, e1, e2
//                 k_kem_encrypt the same device function as above, comparing instead of storing; OR-reduction; masked select
// The roles of k_kem_hash are lane ranges of one launch (task-major: a wave runs one role), longest role first.  Sponge layout by wave
// count: one state per lane, except the two roles that are ONE lane per item with a chain of 6-12 dependent permutations -- H(pk) of an
// encapsulation and rkprf of a decapsulation.  In a launch group of up to KEM_WAVE_MAX items such a role would be a few waves at
// single-wave latency, so it runs as one WAVE per item on the wave sponge (kosk_keccak_wave_dev.hpp), launched ahead of k_kem_hash: H(pk) on
// k_fs_chain<FS_DIGEST> (kosk_fs_kernels.hip), after which the seed role only does G; rkprf on k_kem_rkprf_wave below (SHAKE domain,
// two-part message).  The device functions are in kosk_kem_dev.hpp; DESIGN.md 19 has the resource figures.
//
// crypto_kem_keypair_derand (kem.c:25-35) for batches, in the same shape:
//   key pair      k_kem_kg_hash role   (rho, sigma) = G(d || K)                      one sponge per lane, one lane per item
//                 k_kem_kg_hash roles  gen_matrix (A, not transposed), s, e          (K^2 + 2 K) lanes per item
//                 k_kem_keypair NTT(s), NTT(e), A o s-hat + e-hat, pack pk and sk    one workgroup per item
//                 k_kem_hpk     H(pk) into the sk record                             one lane per item
//   key checks    k_kem_hpk     H(pk inside sk)                                      one lane per item
//                 k_kem_check   12-bit fields >= q, stored H(pk) against the computed one, OR-reduction   one wave per item
// H(pk) is the third one-lane-per-item chain of this file: in a launch group of up to KEM_WAVE_MAX items it runs on k_fs_chain<FS_DIGEST>
// like the encapsulation's, and k_kem_hpk only moves the digest into the record (key pair) or is not launched (checks).
//
// One resident key: what depends on the key alone is decoded once into a slot, the n-item calls do the per-item work only:
//   load          k_kem_key_setup   gen_matrix (A^T), one entry per block; H(pk) on the wave sponge    K^2 + 1 waves, once per key
//   encapsulate   k_kem_hash        role   G(m || h), h from the slot                                 one lane per item
//                 k_kem_hash        roles  r, e1, e2                                                  (2 K + 1) lanes per item
//                 k_kem_encrypt     encrypt_block on the slot's pk and A^T                            one workgroup per item
//   decapsulate   k_kem_decrypt     decrypt_block on the slot's s-hat, G(m' || stored h)              one workgroup per item
//                 k_kem_hash        roles  rkprf (z from the slot; k_kem_rkprf_wave in a small group), r, e1, e2
//                 k_kem_encrypt     comparing
// These are the per-item kernels and the per-item host bodies: a one-key call is the per-item call with every key-side stride 0 (KemKeySide),
// no matrix role and no H(pk).
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "kosk_ctx.hpp"
#include "kosk_keccak_wave_dev.hpp"
#include "kosk_kem_dev.hpp"
#include "kosk_regtree.hpp"

namespace kosk {

using namespace kem;

// HBM workspace of the KEM calls, allocated at a context's first KEM call (a handle that never makes one pays nothing)
struct KemWs {
    int cap = 0;
    uint8_t *d_pk = nullptr, *d_sk = nullptr, *d_ct = nullptr, *d_m = nullptr, *d_kr = nullptr, *d_rk = nullptr, *d_ss = nullptr, *d_mask = nullptr;
    uint8_t *d_h = nullptr; // [n][32] H(pk) from the wave sponge
    int16_t *d_A = nullptr, *d_noise = nullptr;
    int32_t *d_key = nullptr; // [n] the slot of item b (kem_enc_slots), or the slot key b goes to (kem_registry_admit)
};

struct KemHashJob {
    int n, K, eta1;
    int n_rk, n_seed, n_mat, n_noise; // lanes per item of each role, in launch order
    const uint8_t *pk;                // records holding t-hat || rho (the pk, or the pk inside the sk); not read where h is given and n_mat = 0
    size_t pk_stride;
    int pk_bytes;
    const uint8_t *m;                 // [n][32]     seed role: the message
    const uint8_t *h;                 // seed role: H(pk) of item b at h + b * h_stride (wave sponge, or the slot's); nullptr: it hashes pk itself
    size_t h_stride;
    const int32_t *key;               // seed role, with h: item b's H(pk) is that of key key[b]; nullptr: of key b
    uint8_t *kr;                      // [n][64]     seed role writes, noise role reads (coins = kr + 32)
    int16_t *A, *noise;               // [n][K K][256], [n][2 K + 1][256]
    const uint8_t *z;                 // rkprf role: z of item b at z + b * z_stride
    size_t z_stride;
    const uint8_t *ct;                // [n][ct_bytes]
    int ct_bytes;
    uint8_t *rk;                      // [n][32]
    uint32_t *err;
    int max_blocks;
};

__global__ __launch_bounds__(64) void k_kem_hash(KemHashJob j)
{
    const long gid = (long)blockIdx.x * 64 + threadIdx.x;
    const int per = j.n_rk + j.n_seed + j.n_mat + j.n_noise;
    if (gid >= (long)per * j.n) return;
    int t = (int)(gid / j.n);
    const int b = (int)(gid - (long)t * j.n);
    const uint8_t *pk = j.pk + (size_t)b * j.pk_stride;
    if (t < j.n_rk) {
        uint64_t out[4];
        rkprf(j.z + (size_t)b * j.z_stride, j.ct + (size_t)b * j.ct_bytes, j.ct_bytes, out);
#pragma unroll
        for (int l = 0; l < 4; l++) reinterpret_cast<uint64_t *>(j.rk)[4 * (size_t)b + l] = out[l];
        return;
    }
    t -= j.n_rk;
    if (t < j.n_seed) {
        uint64_t m[4], h[4], kr[8];
#pragma unroll
        for (int l = 0; l < 4; l++) m[l] = ld64(j.m, 4 * b + l);
        if (j.h) {
#pragma unroll
            for (int l = 0; l < 4; l++) h[l] = ld64(j.h + (size_t)(j.key ? j.key[b] : b) * j.h_stride, l);
        } else {
            sha3_256_words(pk, j.pk_bytes, h);
        }
        hash_g64(m, h, kr);
#pragma unroll
        for (int l = 0; l < 8; l++) reinterpret_cast<uint64_t *>(j.kr)[8 * (size_t)b + l] = kr[l];
        return;
    }
    t -= j.n_seed;
    if (t < j.n_mat) {
        uint64_t rho[4];
#pragma unroll
        for (int l = 0; l < 4; l++) rho[l] = ld64(pk + j.pk_bytes - 32, l);
        // A^T[i][j] = XOF(rho, i, j) (indcpa.c:177-178)
        if (!matrix_entry(rho, t / j.K, t % j.K, j.max_blocks, j.A + ((size_t)b * j.n_mat + t) * 256))
            if (j.err) *reinterpret_cast<volatile uint32_t *>(j.err) = DEVERR_XOF_BLOCKS;
        return;
    }
    t -= j.n_mat;
    uint64_t coins[4];
#pragma unroll
    for (int l = 0; l < 4; l++) coins[l] = ld64(j.kr, 8 * b + 4 + l);
    noise_poly(coins, t, t < j.K ? j.eta1 : 2, j.noise + ((size_t)b * j.n_noise + t) * 256);
}

// rkprf = SHAKE256(z[32] || ct) (symmetric-shake.c: kyber_shake256_rkprf), one WAVE per item on the wave sponge: a 32-bit half of a state
// word per lane, bit-interleaved (kosk_keccak_wave_dev.hpp, WaveSponge).  z and ct are 8-byte aligned and 32 + ct_bytes is a multiple of 8, so
// every block is whole words.  z is secret: it is data only; the addresses are functions of the lane and the block.
__global__ __launch_bounds__(64) void k_kem_rkprf_wave(const uint8_t *z, size_t z_stride, const uint8_t *ct, int ct_bytes, uint8_t *rk)
{
    __shared__ __align__(16) uint32_t st[64];
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;
    __builtin_amdgcn_s_setprio(3); // a chain is latency, not throughput
    WaveSponge sp;
    sp.setup(lane);
    const uint8_t *zb = z + b * z_stride, *cb = ct + b * (size_t)ct_bytes;
    uint32_t a = 0;
    wave_absorb_words(sp, a, [&](int i) { return *reinterpret_cast<const uint2 *>(i < 4 ? zb + 8 * i : cb + 8 * (i - 4)); }, 4 + ct_bytes / 8, 0x1Fu);
    const uint2 w = sp.words(a, st, 4);
    if (lane < 4) *reinterpret_cast<uint2 *>(rk + b * 32 + 8 * lane) = w;
}

// pk and A^T of item b at pk + kb * pk_stride and A + kb * A_stride (int16_t elements), kb = key[b], or b where key is nullptr: one of each
// per item, the one-key slot's at stride 0, or the registry's by slot
struct KemEncJob {
    int K, dec;
    const uint8_t *pk;
    size_t pk_stride;
    const int16_t *A, *noise;
    size_t A_stride;
    const int32_t *key;
    const uint8_t *m, *kr, *rk; // [n][32], [n][64], [n][32] (dec)
    uint8_t *ct;                // [n][ct_bytes]: written (enc) or compared with (dec)
    uint8_t *ss;                // [n][32]
    const uint8_t *mask;        // enc: optional [n]; 0 = no encapsulation, ct and ss of the item are zero-filled
};

__global__ __launch_bounds__(256) void k_kem_encrypt(KemEncJob j)
{
    __shared__ alignas(16) uint16_t L[9 * 256];
    __shared__ uint32_t fail;
    const Dims D = dims(j.K);
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    uint8_t *ct = j.ct + b * (size_t)D.ct;
    if (j.mask && !j.mask[b]) { // public: the verifier's bit
        for (int i = tid; i < D.ct / 16; i += 256) reinterpret_cast<U128 *>(ct)[i] = U128{0, 0, 0, 0};
        if (tid < 32) j.ss[b * 32 + tid] = 0;
        return;
    }
    if (tid == 0) fail = 0;
    __syncthreads();
    const size_t kb = j.key ? (size_t)j.key[b] : b; // block-uniform: one load
    const uint32_t diff = encrypt_block(D, L, tid, 256, j.pk + kb * j.pk_stride, j.A + kb * j.A_stride,
                                        j.noise + b * (size_t)((2 * D.K + 1) * 256), j.m + b * 32, j.dec ? nullptr : ct, ct);
    if (!j.dec) {
        if (tid < 32) j.ss[b * 32 + tid] = j.kr[b * 64 + tid];
        return;
    }
    atomicOr(&fail, diff);
    __syncthreads();
    if (tid < 32) j.ss[b * 32 + tid] = select_ss(fail, j.kr[b * 64 + tid], j.rk[b * 32 + tid]);
}

// s-hat of item b at shat + b * shat_stride and the H(pk) its sk stored at h + b * h_stride: both inside the item's sk record, or the slot's at
// stride 0.  s-hat, z, m and kr are data only: every address built from them (here and in k_kem_hash, k_kem_rkprf_wave, k_kem_encrypt) is a
// function of the block, the lane and a launch-time stride, whichever caller launched.
struct KemDecJob {
    int K;
    const uint8_t *ct, *shat, *h;
    size_t shat_stride, h_stride;
    uint8_t *m, *kr;
};

__global__ __launch_bounds__(256) void k_kem_decrypt(KemDecJob j)
{
    __shared__ alignas(16) uint16_t L[6 * 256];
    __shared__ alignas(16) uint8_t Lb[288];
    const Dims D = dims(j.K);
    const int tid = threadIdx.x;
    const size_t b = blockIdx.x;
    decrypt_block(D, L, Lb, tid, 256, j.ct + b * (size_t)D.ct, j.shat + b * j.shat_stride);
    if (tid < 32) j.m[b * 32 + tid] = Lb[256 + tid];
    if (tid == 0) {
        uint64_t m[4], h[4], kr[8];
#pragma unroll
        for (int l = 0; l < 4; l++) { m[l] = ld64(Lb + 256, l); h[l] = ld64(j.h + b * j.h_stride, l); }
        hash_g64(m, h, kr);
#pragma unroll
        for (int l = 0; l < 8; l++) reinterpret_cast<uint64_t *>(j.kr)[8 * b + l] = kr[l];
    }
}

// ---- key pairs --------------------------------------------------------------------------------------------------------
struct KemKgJob {
    int n, K, eta1;
    int n_seed, n_mat, n_noise; // lanes per item of each role, in launch order
    const uint8_t *coins;       // [n][64]  d || z
    uint8_t *rho, *sigma;       // [n][32] each: the seed role writes, the other two read
    int16_t *A, *noise;         // [n][K K][256], [n][2 K][256]
    uint32_t *err;
    int max_blocks;
};

__global__ __launch_bounds__(64) void k_kem_kg_hash(KemKgJob j)
{
    const long gid = (long)blockIdx.x * 64 + threadIdx.x;
    const int per = j.n_seed + j.n_mat + j.n_noise;
    if (gid >= (long)per * j.n) return;
    int t = (int)(gid / j.n);
    const int b = (int)(gid - (long)t * j.n);
    if (t < j.n_seed) {
        uint64_t d[4], rs[8];
#pragma unroll
        for (int l = 0; l < 4; l++) d[l] = ld64(j.coins, 8 * b + l);
        seed_hash_g(d, j.K, rs);
#pragma unroll
        for (int l = 0; l < 4; l++) {
            reinterpret_cast<uint64_t *>(j.rho)[4 * (size_t)b + l] = rs[l];
            reinterpret_cast<uint64_t *>(j.sigma)[4 * (size_t)b + l] = rs[4 + l];
        }
        return;
    }
    t -= j.n_seed;
    if (t < j.n_mat) {
        uint64_t rho[4];
#pragma unroll
        for (int l = 0; l < 4; l++) rho[l] = ld64(j.rho, 4 * b + l);
        // A[i][j] = XOF(rho, j, i) (indcpa.c:179-180): entry t = i K + j
        if (!matrix_entry(rho, t % j.K, t / j.K, j.max_blocks, j.A + ((size_t)b * j.n_mat + t) * 256))
            if (j.err) *reinterpret_cast<volatile uint32_t *>(j.err) = DEVERR_XOF_BLOCKS;
        return;
    }
    t -= j.n_mat;
    uint64_t sigma[4];
#pragma unroll
    for (int l = 0; l < 4; l++) sigma[l] = ld64(j.sigma, 4 * b + l);
    noise_poly(sigma, t, j.eta1, j.noise + ((size_t)b * j.n_noise + t) * 256); // s_i: nonce i, e_i: nonce K + i (indcpa.c:225-228)
}

struct KemKeypairJob {
    int K;
    const int16_t *A, *noise;
    const uint8_t *rho, *coins; // [n][32], [n][64]
    uint8_t *pk, *sk;           // [n][pk_bytes], [n][sk_bytes]
};

__global__ __launch_bounds__(256) void k_kem_keypair(KemKeypairJob j)
{
    __shared__ alignas(16) uint16_t L[8 * 256];
    __shared__ alignas(16) uint8_t Lb[768 * 4 + 96];
    const Dims D = dims(j.K);
    const size_t b = blockIdx.x;
    keypair_block(D, L, Lb, threadIdx.x, 256, j.A + b * (size_t)(D.K * D.K * 256), j.noise + b * (size_t)(2 * D.K * 256), j.rho + b * 32,
                  j.coins + b * 64 + 32, j.pk + b * (size_t)D.pk, j.sk + b * (size_t)D.sk);
}

// sha3_256 of record b (`len` bytes at in + b * in_stride, 8-byte aligned), or h[b] where the wave sponge has computed it already, as two
// 16-byte stores to out + b * out_stride (16-byte aligned).  One lane per item.
__global__ __launch_bounds__(64) void k_kem_hpk(int n, const uint8_t *in, size_t in_stride, int len, const uint8_t *h, uint8_t *out, size_t out_stride)
{
    const long b = (long)blockIdx.x * 64 + threadIdx.x;
    if (b >= n) return;
    uint64_t d[4];
    if (h) {
#pragma unroll
        for (int l = 0; l < 4; l++) d[l] = ld64(h, 4 * (int)b + l);
    } else {
        sha3_256_words(in + (size_t)b * in_stride, len, d);
    }
    U128 *o = reinterpret_cast<U128 *>(out + (size_t)b * out_stride);
    o[0] = U128{(uint32_t)d[0], (uint32_t)(d[0] >> 32), (uint32_t)d[1], (uint32_t)(d[1] >> 32)};
    o[1] = U128{(uint32_t)d[2], (uint32_t)(d[2] >> 32), (uint32_t)d[3], (uint32_t)(d[3] >> 32)};
}

// ---- key checks (FIPS 203 7.2, 7.3) -----------------------------------------------------------------------------------
struct KemCheckJob {
    int K, is_sk;
    const uint8_t *rec; // pk records, or sk records (s-hat || pk || H(pk) || z)
    size_t stride;
    const uint8_t *h;   // is_sk: [n][32] sha3_256 of the pk inside record b
    uint8_t *flags;     // [n]
};

// One wave per record.  Every lane looks at groups of eight 12-bit fields (which group is a function of the lane alone); the range
// test is sign-mask arithmetic (range12x8) and the verdict an OR over the wave: no branch and no address depends on s-hat.
__global__ __launch_bounds__(64) void k_kem_check(KemCheckJob j)
{
    __shared__ uint32_t verdict;
    const Dims D = dims(j.K);
    const int lane = threadIdx.x;
    const size_t b = blockIdx.x;
    const uint8_t *rec = j.rec + b * j.stride;
    if (lane == 0) verdict = 0;
    __syncthreads();
    uint32_t f = 0;
    const int per = D.K * 32; // groups per polyvec; in an sk the pk's follow s-hat's directly
    for (int w = lane; w < (j.is_sk ? 2 : 1) * per; w += 64)
        f |= range12x8(rec + 12 * w) * (j.is_sk && w < per ? (uint32_t)KEYCHK_S_RANGE : (uint32_t)KEYCHK_PK_RANGE);
    if (j.is_sk && lane < 32) f |= nonzero_bit((uint32_t)(j.h[b * 32 + lane] ^ rec[D.sk - 64 + lane])) * (uint32_t)KEYCHK_HASH;
    atomicOr(&verdict, f);
    __syncthreads();
    if (lane == 0) j.flags[b] = (uint8_t)verdict;
}

// ---- one resident key ------------------------------------------------------------------------------------
// The slot: what depends on the key alone, decoded once by k_kem_key_setup and read by every item of every later call.  Two allocations of
// its own (kem_ensure frees and reallocates the workspace above; the slot must not move), filed in the inventory under INVG_KEMKEY:
//   d_pub (public)  pk [384 K + 32] | H(pk) of those bytes [32] | the H(pk) stored in the sk [32] | A^T [K][K][256] int16
//   d_sec (secret)  s-hat [384 K] | z [32]
struct KemKey {
    int state = KEM_KEY_NONE;
    bool wiped = false; // loaded from an sk, then wipe_secrets() zeroed d_sec: decapsulation refuses, encapsulation goes on
    uint8_t *d_pub = nullptr, *d_sec = nullptr;
    uint8_t *pk = nullptr, *h_enc = nullptr, *h_dec = nullptr, *shat = nullptr, *z = nullptr;
    int16_t *A = nullptr;
};

// Blocks 0 .. K K - 1: entry (i, j) of A^T, one sponge on lane 0 (three or four dependent permutations; the K K entries run side by side).
// Block K K: H(pk), the longer chain (6 / 9 / 12 permutations for K = 2 / 3 / 4), on the wave sponge.  One key, one launch: both at
// single-wave latency, so the long chain gets the layout whose permutation is short.  pk: 16-byte aligned, pk_bytes a multiple of 8.
__global__ __launch_bounds__(64) void k_kem_key_setup(int K, const uint8_t *pk, int pk_bytes, int16_t *A, uint8_t *h, uint32_t *err, int max_blocks)
{
    __shared__ __align__(16) uint32_t st[64];
    const int lane = threadIdx.x, t = blockIdx.x;
    if (t < K * K) { // block-uniform
        if (lane) return;
        uint64_t rho[4];
#pragma unroll
        for (int l = 0; l < 4; l++) rho[l] = ld64(pk + pk_bytes - 32, l);
        // A^T[i][j] = XOF(rho, i, j) (indcpa.c:177-178), as the matrix role of k_kem_hash
        if (!matrix_entry(rho, t / K, t % K, max_blocks, A + (size_t)t * 256))
            if (err) *reinterpret_cast<volatile uint32_t *>(err) = DEVERR_XOF_BLOCKS;
        return;
    }
    __builtin_amdgcn_s_setprio(3);
    WaveSponge sp;
    sp.setup(lane);
    uint32_t a = 0;
    wave_absorb_words(sp, a, [&](int i) { return *reinterpret_cast<const uint2 *>(pk + 8 * i); }, pk_bytes / 8, 0x06u);
    const uint2 w = sp.words(a, st, 4);
    if (lane < 4) *reinterpret_cast<uint2 *>(h + 8 * lane) = w;
}

// ---------------------------------------------------------------------------------------------------------------- host --
#define HIPCHK(x) KOSK_HIPCHK(x)

void kem_release(Ctx &c)
{
    KemWs *w = c.kem;
    if (!w) return;
    c.inv.release(Inventory::INVG_KEM);
    delete w;
    c.kem = nullptr;
}

// the workspace holds the largest launch group the context has seen (rounded up to 1 024 items, at most KEM_CHUNK)
static int kem_ensure(Ctx &c, int n)
{
    if (c.kem && c.kem->cap >= n) return 0;
    if (c.kem) {
        KOSK_HIPCHK(stream_sync(c));
        if (wipe_group(c, Inventory::INVG_KEM)) return -1; // the workspace of the earlier calls does not go back to the allocator readable
        kem_release(c);
    }
    const Dims D = dims(c.P.K);
    KemWs *w = new KemWs();
    c.kem = w;
    const size_t N = (size_t)((n + 1023) / 1024 * 1024 < KEM_CHUNK ? (n + 1023) / 1024 * 1024 : KEM_CHUNK);
    // secret are the records, messages, hashes of them and the noise; public the keys, ciphertexts, A, H(pk), flags
    const int S = Inventory::INV_SECRET, G = Inventory::INVG_KEM;
    auto body = [&]() -> int {
        HIPCHK(hipSetDevice(c.device));
        HIPCHK(c.own("kem.d_sk", &w->d_sk, N * D.sk, S, G));
        HIPCHK(c.own("kem.d_m", &w->d_m, N * 32, S, G));
        HIPCHK(c.own("kem.d_kr", &w->d_kr, N * 64, S, G));
        HIPCHK(c.own("kem.d_rk", &w->d_rk, N * 32, S, G));
        HIPCHK(c.own("kem.d_ss", &w->d_ss, N * 32, S, G));
        HIPCHK(c.own("kem.d_noise", &w->d_noise, N * (2 * D.K + 1) * 512, S, G));
        HIPCHK(c.own("kem.d_pk", &w->d_pk, N * D.pk, 0, G));
        HIPCHK(c.own("kem.d_ct", &w->d_ct, N * D.ct, 0, G));
        HIPCHK(c.own("kem.d_mask", &w->d_mask, N, 0, G));
        HIPCHK(c.own("kem.d_h", &w->d_h, N * 32, 0, G));
        HIPCHK(c.own("kem.d_A", &w->d_A, N * D.K * D.K * 512, 0, G));
        HIPCHK(c.own("kem.d_key", &w->d_key, N * sizeof(int32_t), 0, G));
        return 0;
    };
    if (body()) { kem_release(c); return -1; }
    w->cap = (int)N;
    return 0;
}

static hipError_t kem_copy_in(Ctx &c, void *d_dst, const void *src, size_t bytes)
{
    return hipMemcpyAsync(d_dst, src, bytes, is_device_pointer(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c.stream);
}
static hipError_t kem_copy_out(Ctx &c, void *dst, const void *d_src, size_t bytes)
{
    return hipMemcpyAsync(dst, d_src, bytes, is_device_pointer(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c.stream);
}
// KOSK_DEBUG_KEM_WAVE_MAX=n moves the boundary between the two sponge layouts (tests run the per-lane roles on small batches with 0)
static int kem_wave_max()
{
    static const int v = [] { const char *e = getenv("KOSK_DEBUG_KEM_WAVE_MAX"); return e ? atoi(e) : (int)KEM_WAVE_MAX; }();
    return v;
}
static hipError_t kem_launch_hash(const KemHashJob &j, hipStream_t st)
{
    const long lanes = (long)(j.n_rk + j.n_seed + j.n_mat + j.n_noise) * j.n;
    k_kem_hash<<<dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, st>>>(j);
    return hipGetLastError();
}

// H(pk) of n records under the two-layout rule: up to kem_wave_max() items one wave per item into w.d_h (returns true: the caller
// takes it from there), above that nothing is launched and the caller's one-lane-per-item kernel hashes (returns false)
static int kem_hpk_wave(Ctx &c, int n, const uint8_t *in, size_t in_stride, int len, bool &done)
{
    done = n <= kem_wave_max();
    if (!done) return 0;
    FsArgs fa{};
    fa.in = in; fa.in_stride = in_stride; fa.len = len; fa.out_digest = c.kem->d_h;
    HIPCHK(launch_fs_chain(fa, FS_DIGEST, n, c.stream));
    return 0;
}

// The key side of a KEM call: item b's piece of the key lies at base + b * stride.  The per-item calls point it into the workspace (or at
// the resident verified keys), where A^T and H(pk) are still to be computed; a one-key call points it at the slot, every stride 0; a call by
// slot points it at the registry with the index `key` (device memory): item b's pieces then lie at base + key[b] * stride.  Only the seed role of
// k_kem_hash (h_enc) and k_kem_encrypt (pk, A) read the index.
struct KemKeySide {
    const uint8_t *pk, *h_enc, *shat, *h_dec, *z; // h_enc: H(pk) for G of an encapsulation; h_dec: the H(pk) stored in the sk
    const int16_t *A;
    size_t pk_stride, h_enc_stride, shat_stride, h_dec_stride, z_stride, A_stride; // A_stride in int16_t elements
    const int32_t *key;                           // nullptr: item b uses key b
    bool derive;                                  // A^T (matrix role, into A) and H(pk) (kem_wave_max() rule, into h_enc) belong to the call
    bool h_ready;                                 // with derive: a kernel queued on the stream has written H(pk) to h_enc already (kem_enc_proven)
};

// n records at `rec`, `stride` bytes apart: public keys, or (is_sk) secret keys s-hat || pk || H(pk) || z
static KemKeySide kem_side_items(const KemWs &w, const Dims &D, const uint8_t *rec, size_t stride, bool is_sk)
{
    KemKeySide k{};
    k.pk = is_sk ? rec + D.pvb : rec; k.pk_stride = stride;
    k.A = w.d_A; k.A_stride = (size_t)D.K * D.K * 256;
    k.h_enc = w.d_h; k.h_enc_stride = 32;
    if (is_sk) {
        k.shat = rec; k.h_dec = rec + D.sk - 64; k.z = rec + D.sk - 32;
        k.shat_stride = k.h_dec_stride = k.z_stride = stride;
    }
    k.derive = true;
    return k;
}

static KemKeySide kem_side_slot(const KemKey &s)
{
    KemKeySide k{};
    k.pk = s.pk; k.A = s.A; k.h_enc = s.h_enc; k.shat = s.shat; k.h_dec = s.h_dec; k.z = s.z;
    return k;
}

static KemHashJob kem_hash_job(Ctx &c, int n, const KemKeySide &k)
{
    KemWs &w = *c.kem;
    const Dims D = dims(c.P.K);
    KemHashJob h{};
    h.n = n; h.K = D.K; h.eta1 = D.eta1;
    h.pk = k.pk; h.pk_stride = k.pk_stride; h.pk_bytes = D.pk;
    h.kr = w.d_kr; h.A = w.d_A; h.noise = w.d_noise;
    h.err = c.h_err; h.max_blocks = c.xof_max_blocks;
    return h;
}

static hipError_t kem_launch_encrypt(Ctx &c, int n, const KemKeySide &k, int dec, const uint8_t *d_mask)
{
    KemWs &w = *c.kem;
    KemEncJob e{};
    e.K = c.P.K; e.dec = dec; e.pk = k.pk; e.pk_stride = k.pk_stride; e.A = k.A; e.A_stride = k.A_stride; e.key = k.key; e.noise = w.d_noise;
    e.m = w.d_m; e.kr = w.d_kr; e.rk = dec ? w.d_rk : nullptr; e.ct = w.d_ct; e.ss = w.d_ss; e.mask = d_mask;
    k_kem_encrypt<<<dim3((unsigned)n), dim3(256), 0, c.stream>>>(e);
    return hipGetLastError();
}

// Encapsulation under either key side (the workspace holds n items): `path` is the caller's path_n[] counter.  mask: host memory, or
// w.d_mask itself where a kernel queued on the stream has written it already (kem_enc_peers): nothing is copied then
static int kem_enc_body(Ctx &c, int n, const KemKeySide &k, const uint8_t *coins, uint8_t *ct, uint8_t *ss, const uint8_t *mask, int path)
{
    KemWs &w = *c.kem;
    const Dims D = dims(c.P.K);
    HIPCHK(kem_copy_in(c, w.d_m, coins, (size_t)n * 32));
    if (mask && mask != w.d_mask) HIPCHK(hipMemcpyAsync(w.d_mask, mask, (size_t)n, hipMemcpyHostToDevice, c.stream));
    KemHashJob h = kem_hash_job(c, n, k);
    h.m = w.d_m; h.h = k.h_enc; h.h_stride = k.h_enc_stride; h.key = k.key;
    if (k.derive) {
        if (!k.h_ready) {
            bool wave = false; // H(pk): one wave per key on the wave sponge, or the seed role hashes pk itself
            if (kem_hpk_wave(c, n, k.pk, k.pk_stride, D.pk, wave)) return -1;
            if (!wave) h.h = nullptr;
        }
        h.n_mat = D.K * D.K;
    }
    h.n_seed = 1;
    HIPCHK(kem_launch_hash(h, c.stream));
    h.n_seed = 0; h.n_mat = 0; h.n_noise = 2 * D.K + 1;
    HIPCHK(kem_launch_hash(h, c.stream));
    HIPCHK(kem_launch_encrypt(c, n, k, 0, mask ? w.d_mask : nullptr));
    c.path_n[path]++;
    if (k.derive) {
        HIPCHK(stream_sync(c));
        if (device_error_check(c)) return -1; // gen_matrix block limit: no results
    }
    HIPCHK(kem_copy_out(c, ct, w.d_ct, (size_t)n * D.ct));
    HIPCHK(kem_copy_out(c, ss, w.d_ss, (size_t)n * 32));
    HIPCHK(stream_sync(c));
    return 0;
}

// Decapsulation of the n ciphertexts in w.d_ct under either key side
static int kem_dec_body(Ctx &c, int n, const KemKeySide &k, uint8_t *ss, int path)
{
    KemWs &w = *c.kem;
    const Dims D = dims(c.P.K);
    KemDecJob d{};
    d.K = D.K; d.ct = w.d_ct; d.shat = k.shat; d.shat_stride = k.shat_stride; d.h = k.h_dec; d.h_stride = k.h_dec_stride; d.m = w.d_m; d.kr = w.d_kr;
    k_kem_decrypt<<<dim3((unsigned)n), dim3(256), 0, c.stream>>>(d);
    HIPCHK(hipGetLastError());
    KemHashJob h = kem_hash_job(c, n, k);
    h.z = k.z; h.z_stride = k.z_stride; h.ct = w.d_ct; h.ct_bytes = D.ct; h.rk = w.d_rk;
    h.n_rk = 1; h.n_mat = k.derive ? D.K * D.K : 0; h.n_noise = 2 * D.K + 1;
    if (n <= kem_wave_max()) { // rkprf: one wave per item on the wave sponge
        k_kem_rkprf_wave<<<dim3((unsigned)n), dim3(64), 0, c.stream>>>(h.z, h.z_stride, h.ct, h.ct_bytes, h.rk);
        HIPCHK(hipGetLastError());
        h.n_rk = 0;
    }
    HIPCHK(kem_launch_hash(h, c.stream));
    HIPCHK(kem_launch_encrypt(c, n, k, 1, nullptr));
    c.path_n[path]++;
    if (k.derive) {
        HIPCHK(stream_sync(c));
        if (device_error_check(c)) return -1;
    }
    HIPCHK(kem_copy_out(c, ss, w.d_ss, (size_t)n * 32));
    HIPCHK(stream_sync(c));
    return 0;
}

int kem_enc(Ctx &c, int n, const uint8_t *pk, const uint8_t *coins, uint8_t *ct, uint8_t *ss, const uint8_t *mask, int resident_first)
{
    if (n < 1 || n > KEM_CHUNK || !coins || !ct || !ss) { c.err = "kem_enc: bad arguments"; return -1; }
    if (kem_ensure(c, n)) return -1;
    KemWs &w = *c.kem;
    const Dims D = dims(c.P.K);
    HIPCHK(hipSetDevice(c.device));
    const uint8_t *d_pk = w.d_pk;
    size_t pk_stride = (size_t)D.pk;
    if (pk) HIPCHK(kem_copy_in(c, w.d_pk, pk, (size_t)n * D.pk));
    else { d_pk = c.d_pk + (size_t)resident_first * c.pk_stride; pk_stride = c.pk_stride; } // the keys the last verify call left resident (kosk_kem_enc_verified)
    return kem_enc_body(c, n, kem_side_items(w, D, d_pk, pk_stride, false), coins, ct, ss, mask, PATH_KEM_ENC);
}

int kem_dec(Ctx &c, int n, const uint8_t *ct, const uint8_t *sk, uint8_t *ss)
{
    if (n < 1 || n > KEM_CHUNK || !ct || !sk || !ss) { c.err = "kem_dec: bad arguments"; return -1; }
    if (kem_ensure(c, n)) return -1;
    KemWs &w = *c.kem;
    const Dims D = dims(c.P.K);
    HIPCHK(hipSetDevice(c.device));
    HIPCHK(kem_copy_in(c, w.d_ct, ct, (size_t)n * D.ct));
    HIPCHK(kem_copy_in(c, w.d_sk, sk, (size_t)n * D.sk));
    return kem_dec_body(c, n, kem_side_items(w, D, w.d_sk, (size_t)D.sk, true), ss, PATH_KEM_DEC);
}

int kem_keypair(Ctx &c, int n, const uint8_t *coins, uint8_t *pk, uint8_t *sk)
{
    if (n < 1 || n > KEM_CHUNK || !coins || !pk || !sk) { c.err = "kem_keypair: bad arguments"; return -1; }
    if (kem_ensure(c, n)) return -1;
    KemWs &w = *c.kem;
    const Dims D = dims(c.P.K);
    HIPCHK(hipSetDevice(c.device));
    // workspace roles: d_kr coins (d || z), d_m rho, d_rk sigma, d_A A, d_noise s | e, d_pk / d_sk the records, d_h H(pk)
    HIPCHK(kem_copy_in(c, w.d_kr, coins, (size_t)n * 64));
    KemKgJob h{};
    h.n = n; h.K = D.K; h.eta1 = D.eta1;
    h.coins = w.d_kr; h.rho = w.d_m; h.sigma = w.d_rk; h.A = w.d_A; h.noise = w.d_noise;
    h.err = c.h_err; h.max_blocks = c.xof_max_blocks;
    auto launch = [&]() {
        const long lanes = (long)(h.n_seed + h.n_mat + h.n_noise) * n;
        k_kem_kg_hash<<<dim3((unsigned)((lanes + 63) / 64)), dim3(64), 0, c.stream>>>(h);
        return hipGetLastError();
    };
    h.n_seed = 1;
    HIPCHK(launch());
    h.n_seed = 0; h.n_mat = D.K * D.K; h.n_noise = 2 * D.K;
    HIPCHK(launch());
    KemKeypairJob k{};
    k.K = D.K; k.A = w.d_A; k.noise = w.d_noise; k.rho = w.d_m; k.coins = w.d_kr; k.pk = w.d_pk; k.sk = w.d_sk;
    k_kem_keypair<<<dim3((unsigned)n), dim3(256), 0, c.stream>>>(k);
    HIPCHK(hipGetLastError());
    bool wave = false;
    if (kem_hpk_wave(c, n, w.d_pk, (size_t)D.pk, D.pk, wave)) return -1;
    k_kem_hpk<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c.stream>>>(n, w.d_pk, (size_t)D.pk, D.pk, wave ? w.d_h : nullptr, w.d_sk + D.sk - 64, (size_t)D.sk);
    HIPCHK(hipGetLastError());
    c.path_n[PATH_KEM_KEYPAIR]++;
    HIPCHK(stream_sync(c));
    if (device_error_check(c)) return -1; // gen_matrix block limit: no results
    HIPCHK(kem_copy_out(c, pk, w.d_pk, (size_t)n * D.pk));
    HIPCHK(kem_copy_out(c, sk, w.d_sk, (size_t)n * D.sk));
    HIPCHK(stream_sync(c));
    return 0;
}

int kem_check(Ctx &c, int n, const uint8_t *rec, int is_sk, uint8_t *flags)
{
    if (n < 1 || n > KEM_CHUNK || !rec || !flags) { c.err = "kem_check: bad arguments"; return -1; }
    if (kem_ensure(c, n)) return -1;
    KemWs &w = *c.kem;
    const Dims D = dims(c.P.K);
    HIPCHK(hipSetDevice(c.device));
    KemCheckJob k{};
    k.K = D.K; k.is_sk = is_sk; k.flags = w.d_mask;
    if (is_sk) {
        HIPCHK(kem_copy_in(c, w.d_sk, rec, (size_t)n * D.sk));
        k.rec = w.d_sk; k.stride = (size_t)D.sk; k.h = w.d_h;
        bool wave = false;
        if (kem_hpk_wave(c, n, w.d_sk + D.pvb, (size_t)D.sk, D.pk, wave)) return -1;
        if (!wave) {
            k_kem_hpk<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c.stream>>>(n, w.d_sk + D.pvb, (size_t)D.sk, D.pk, nullptr, w.d_h, 32);
            HIPCHK(hipGetLastError());
        }
    } else {
        HIPCHK(kem_copy_in(c, w.d_pk, rec, (size_t)n * D.pk));
        k.rec = w.d_pk; k.stride = (size_t)D.pk;
    }
    k_kem_check<<<dim3((unsigned)n), dim3(64), 0, c.stream>>>(k);
    HIPCHK(hipGetLastError());
    c.path_n[PATH_KEM_CHECK]++;
    HIPCHK(kem_copy_out(c, flags, w.d_mask, (size_t)n));
    HIPCHK(stream_sync(c));
    return 0;
}

// ---- one resident key ----------------------------------------------------------------------------------------------------
void kem_key_release(Ctx &c)
{
    KemKey *k = c.kem_key;
    if (!k) return;
    c.inv.release(Inventory::INVG_KEMKEY);
    delete k;
    c.kem_key = nullptr;
}

int kem_key_state(const Ctx &c) { return c.kem_key ? c.kem_key->state : (int)KEM_KEY_NONE; }

void kem_key_note_wiped(Ctx &c)
{
    KemKey *k = c.kem_key;
    if (k && k->state == KEM_KEY_SK) { k->state = KEM_KEY_PK; k->wiped = true; }
}

int kem_key_clear(Ctx &c)
{
    if (!c.kem_key) return 0;
    HIPCHK(hipSetDevice(c.device));
    HIPCHK(stream_sync(c));
    const int rc = wipe_group(c, Inventory::INVG_KEMKEY); // s-hat and z do not go back to the allocator readable
    kem_key_release(c);
    return rc;
}

int kem_key_set(Ctx &c, const uint8_t *pk, const uint8_t *sk)
{
    if ((pk == nullptr) == (sk == nullptr)) { c.err = "kem_key_set: exactly one of pk / sk"; return -1; }
    if (kem_key_clear(c)) return -1; // a second load replaces the slot: the old one is wiped first
    const Dims D = dims(c.P.K);
    HIPCHK(hipSetDevice(c.device));
    KemKey *k = new KemKey();
    c.kem_key = k;
    const size_t pub_bytes = (size_t)D.pk + 64 + (size_t)D.K * D.K * 512, sec_bytes = (size_t)D.pvb + 32;
    auto body = [&]() -> int {
        HIPCHK(c.own("kemkey.pub", &k->d_pub, pub_bytes, 0, Inventory::INVG_KEMKEY));
        HIPCHK(c.own("kemkey.sec", &k->d_sec, sec_bytes, Inventory::INV_SECRET, Inventory::INVG_KEMKEY));
        k->pk = k->d_pub; k->h_enc = k->d_pub + D.pk; k->h_dec = k->h_enc + 32; // D.pk is a multiple of 16: A^T stays 16-byte aligned
        k->A = reinterpret_cast<int16_t *>(k->h_dec + 32);
        k->shat = k->d_sec; k->z = k->d_sec + D.pvb;
        HIPCHK(hipMemsetAsync(k->d_pub, 0, pub_bytes, c.stream));
        HIPCHK(hipMemsetAsync(k->d_sec, 0, sec_bytes, c.stream));
        if (sk) { // sk = s-hat || pk || H(pk) || z: the pieces go straight to their places, no copy of the record in between
            HIPCHK(kem_copy_in(c, k->shat, sk, (size_t)D.pvb));
            HIPCHK(kem_copy_in(c, k->pk, sk + D.pvb, (size_t)D.pk));
            HIPCHK(kem_copy_in(c, k->h_dec, sk + D.sk - 64, 32));
            HIPCHK(kem_copy_in(c, k->z, sk + D.sk - 32, 32));
        } else {
            HIPCHK(kem_copy_in(c, k->pk, pk, (size_t)D.pk));
        }
        k_kem_key_setup<<<dim3((unsigned)(D.K * D.K + 1)), dim3(64), 0, c.stream>>>(D.K, k->pk, D.pk, k->A, k->h_enc, c.h_err, c.xof_max_blocks);
        HIPCHK(hipGetLastError());
        c.path_n[PATH_KEM_KEY_SETUP]++;
        HIPCHK(stream_sync(c));
        return device_error_check(c); // gen_matrix block limit: no key
    };
    if (body()) {
        const std::string why = c.err;
        (void)kem_key_clear(c); // the slot stays empty
        c.err = why;
        return -1;
    }
    k->state = sk ? KEM_KEY_SK : KEM_KEY_PK;
    return 0;
}

int kem_enc_key(Ctx &c, int n, const uint8_t *coins, uint8_t *ct, uint8_t *ss)
{
    if (n < 1 || n > KEM_CHUNK || !coins || !ct || !ss) { c.err = "kem_enc_key: bad arguments"; return -1; }
    if (kem_key_state(c) == KEM_KEY_NONE) { c.err = "kem_enc_key: no key is loaded (kosk_kem_key_set)"; return -1; }
    if (kem_ensure(c, n)) return -1;
    HIPCHK(hipSetDevice(c.device));
    return kem_enc_body(c, n, kem_side_slot(*c.kem_key), coins, ct, ss, nullptr, PATH_KEM_ENC_KEY);
}

int kem_dec_key(Ctx &c, int n, const uint8_t *ct, uint8_t *ss)
{
    if (n < 1 || n > KEM_CHUNK || !ct || !ss) { c.err = "kem_dec_key: bad arguments"; return -1; }
    if (kem_key_state(c) != KEM_KEY_SK) {
        c.err = c.kem_key && c.kem_key->wiped ? "kem_dec_key: key was wiped (kosk_wipe_secrets): load the secret key again"
                : c.kem_key               ? "kem_dec_key: the loaded key is a public key"
                                          : "kem_dec_key: no key is loaded (kosk_kem_key_set)";
        return -1;
    }
    if (kem_ensure(c, n)) return -1;
    HIPCHK(hipSetDevice(c.device));
    HIPCHK(kem_copy_in(c, c.kem->d_ct, ct, (size_t)n * dims(c.P.K).ct));
    return kem_dec_body(c, n, kem_side_slot(*c.kem_key), ss, PATH_KEM_DEC_KEY);
}

// ---- the verified-key registry (kosk_registry.hip) ----------------------------------------------------------
int kem_registry_admit(Ctx &c, int n, const uint8_t *pk, int resident_first, const int32_t *slots)
{
    if (n < 1 || n > KEM_CHUNK || !slots || !c.registry) { c.err = "kem_registry_admit: bad arguments"; return -1; }
    if (kem_ensure(c, n)) return -1;
    KemWs &w = *c.kem;
    KemRegistry &r = *c.registry;
    const Dims D = dims(c.P.K);
    HIPCHK(hipSetDevice(c.device));
    r.lookups_stale(); // the next lookup rebuilds the fingerprint index, the next proof of absence the sorted tree
    r.tree_valid = false;  // and the next tree call the leaf subtrees of these slots (a registry without a tree has no bitmap: nothing to walk)
    if (uint8_t *dirty = r.dirty.empty() ? nullptr : r.dirty.data())
        for (int b = 0; b < n; b++)
            if (slots[b] >= 0) dirty[slots[b] >> regtree::TIER_LEVELS] = 1;
    RegAdmitJob j{};
    j.n = n; j.K = D.K; j.pk_bytes = D.pk; j.wave = n <= kem_wave_max();
    if (pk) { // the records through the workspace: 16-byte aligned whatever the caller's pointer is
        HIPCHK(kem_copy_in(c, w.d_pk, pk, (size_t)n * D.pk));
        j.src = w.d_pk; j.src_stride = (size_t)D.pk;
    } else {  // the keys the last verify call left resident (kosk_registry_admit_verified)
        j.src = c.d_pk + (size_t)resident_first * c.pk_stride; j.src_stride = c.pk_stride;
    }
    HIPCHK(hipMemcpyAsync(w.d_key, slots, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c.stream));
    j.slot = w.d_key; j.pk = r.d_pk; j.h = r.d_h; j.flag = r.d_flag; j.A = r.d_A;
    j.err = c.h_err; j.max_blocks = c.xof_max_blocks;
    HIPCHK(launch_registry_admit(j, c.stream));
    c.path_n[PATH_REGISTRY_ADMIT]++;
    // the staged copy goes: after an eviction no byte of the key is left in the handle's HBM
    if (pk) HIPCHK(hipMemsetAsync(w.d_pk, 0, (size_t)n * D.pk, c.stream));
    HIPCHK(stream_sync(c));
    return device_error_check(c); // gen_matrix block limit: the caller empties the slots
}

int kem_enc_slots(Ctx &c, int n, const int32_t *slots, const uint8_t *coins, uint8_t *ct, uint8_t *ss)
{
    if (n < 1 || n > KEM_CHUNK || !slots || !coins || !ct || !ss || !c.registry) { c.err = "kem_enc_slots: bad arguments"; return -1; }
    if (kem_ensure(c, n)) return -1;
    KemWs &w = *c.kem;
    const KemRegistry &r = *c.registry;
    const Dims D = dims(c.P.K);
    HIPCHK(hipSetDevice(c.device));
    std::vector<uint8_t> mask((size_t)n); // the occupancy mirror: an empty slot's ct and ss are zero-filled
    bool all = true;
    for (int b = 0; b < n; b++) all &= (mask[(size_t)b] = r.occ[(size_t)slots[b]]) != 0;
    HIPCHK(hipMemcpyAsync(w.d_key, slots, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c.stream));
    KemKeySide k{};
    k.pk = r.d_pk; k.pk_stride = (size_t)D.pk;
    k.h_enc = r.d_h; k.h_enc_stride = 32;
    k.A = r.d_A; k.A_stride = (size_t)D.K * D.K * 256;
    k.key = w.d_key;
    return kem_enc_body(c, n, k, coins, ct, ss, all ? nullptr : mask.data(), PATH_KEM_ENC_SLOTS);
}

// ---- the registry by fingerprint (kosk_registry.hip) --------------------------------------------------------
// k_registry_find on the n fingerprints staged in w.d_h, queued: the slots into `slot` (or nullptr), and with enc the pair the KEM kernels
// read into w.d_key / w.d_mask
static int kem_launch_find(Ctx &c, int n, int32_t *slot, bool enc)
{
    KemWs &w = *c.kem;
    const KemRegistry &r = *c.registry;
    RegFindJob f{};
    f.n = n; f.capacity = r.capacity; f.mask = (uint32_t)(registry_index_entries(r.capacity) - 1);
    f.q = w.d_h; f.h = r.d_h; f.index = r.d_index; f.slot = slot; f.err = c.h_err;
    if (enc) { f.key = w.d_key; f.found = w.d_mask; }
    HIPCHK(launch_registry_find(f, c.stream));
    c.path_n[PATH_REGISTRY_FIND]++;
    return 0;
}

int kem_registry_find(Ctx &c, int n, const uint8_t *h, int32_t *slots)
{
    if (n < 1 || n > KEM_CHUNK || !h || !slots || !c.registry) { c.err = "kem_registry_find: bad arguments"; return -1; }
    if (kem_ensure(c, n)) return -1;
    if (registry_index_ensure(c)) return -1;
    KemWs &w = *c.kem;
    HIPCHK(hipSetDevice(c.device));
    HIPCHK(kem_copy_in(c, w.d_h, h, (size_t)n * 32)); // through the workspace: 16-byte aligned whatever the caller's pointer is
    if (kem_launch_find(c, n, w.d_key, false)) return -1;
    HIPCHK(hipMemsetAsync(w.d_h, 0, (size_t)n * 32, c.stream)); // the staged fingerprints go: an evicted key leaves no hash behind
    HIPCHK(kem_copy_out(c, slots, w.d_key, (size_t)n * sizeof(int32_t)));
    HIPCHK(stream_sync(c));
    return device_error_check(c); // index overflow
}

int kem_registry_probe(Ctx &c, int n, const uint8_t *pk, int resident_first, uint8_t *h, int32_t *hit)
{
    if (n < 1 || n > KEM_CHUNK || !h || !hit || !c.registry) { c.err = "kem_registry_probe: bad arguments"; return -1; }
    if (kem_ensure(c, n)) return -1;
    if (registry_index_ensure(c)) return -1;
    KemWs &w = *c.kem;
    const Dims D = dims(c.P.K);
    HIPCHK(hipSetDevice(c.device));
    const uint8_t *src = w.d_pk;
    size_t stride = (size_t)D.pk;
    if (pk) HIPCHK(kem_copy_in(c, w.d_pk, pk, (size_t)n * D.pk));
    else { src = c.d_pk + (size_t)resident_first * c.pk_stride; stride = c.pk_stride; } // the keys the last verify call left resident
    bool wave = false; // H(pk) under the two-layout rule, into w.d_h either way
    if (kem_hpk_wave(c, n, src, stride, D.pk, wave)) return -1;
    if (!wave) {
        k_kem_hpk<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c.stream>>>(n, src, stride, D.pk, nullptr, w.d_h, 32);
        HIPCHK(hipGetLastError());
    }
    if (kem_launch_find(c, n, w.d_key, false)) return -1;
    HIPCHK(hipMemcpyAsync(h, w.d_h, (size_t)n * 32, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipMemcpyAsync(hit, w.d_key, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c.stream));
    // the staged copies go, as in kem_registry_admit
    if (pk) HIPCHK(hipMemsetAsync(w.d_pk, 0, (size_t)n * D.pk, c.stream));
    HIPCHK(hipMemsetAsync(w.d_h, 0, (size_t)n * 32, c.stream));
    HIPCHK(stream_sync(c));
    return device_error_check(c);
}

int kem_enc_peers(Ctx &c, int n, const uint8_t *h, const uint8_t *coins, uint8_t *ct, uint8_t *ss, uint8_t *done)
{
    if (n < 1 || n > KEM_CHUNK || !h || !coins || !ct || !ss || !done || !c.registry) { c.err = "kem_enc_peers: bad arguments"; return -1; }
    if (kem_ensure(c, n)) return -1;
    if (registry_index_ensure(c)) return -1;
    KemWs &w = *c.kem;
    const KemRegistry &r = *c.registry;
    const Dims D = dims(c.P.K);
    HIPCHK(hipSetDevice(c.device));
    HIPCHK(kem_copy_in(c, w.d_h, h, (size_t)n * 32));
    if (kem_launch_find(c, n, nullptr, true)) return -1; // the slot index and the mask stay in HBM
    HIPCHK(hipMemsetAsync(w.d_h, 0, (size_t)n * 32, c.stream));
    HIPCHK(kem_copy_out(c, done, w.d_mask, (size_t)n)); // queued here: the body's last synchronisation covers it
    KemKeySide k{};
    k.pk = r.d_pk; k.pk_stride = (size_t)D.pk;
    k.h_enc = r.d_h; k.h_enc_stride = 32;
    k.A = r.d_A; k.A_stride = (size_t)D.K * D.K * 256;
    k.key = w.d_key;
    if (kem_enc_body(c, n, k, coins, ct, ss, w.d_mask, PATH_KEM_ENC_PEERS)) return -1;
    return device_error_check(c); // index overflow
}

// ---- the relying party (kosk_relying.hip) -------------------------------------------------------------------
int kem_enc_proven(Ctx &c, int n, int D, const uint8_t *pk, const int32_t *slots, const uint8_t *paths, const uint8_t *root, const uint8_t *coins,
                   uint8_t *ct, uint8_t *ss, uint8_t *done)
{
    if (n < 1 || n > KEM_CHUNK || D < 0 || D > 31 || !pk || !slots || (D > 0 && !paths) || !root || !coins || !ct || !ss || !done) { c.err = "kem_enc_proven: bad arguments"; return -1; }
    if (kem_ensure(c, n)) return -1;
    if (relying_ensure(c, n, (size_t)D * 32)) return -1;
    KemWs &w = *c.kem;
    const Dims Dm = dims(c.P.K);
    HIPCHK(hipSetDevice(c.device));
    HIPCHK(kem_copy_in(c, w.d_pk, pk, (size_t)n * Dm.pk));
    HIPCHK(kem_copy_in(c, c.d_rl_slot, slots, (size_t)n * sizeof(int32_t)));
    if (D > 0) HIPCHK(kem_copy_in(c, c.d_rl_rec, paths, (size_t)n * D * 32));
    bool wave = false; // H(pk) under the two-layout rule, into w.d_h either way: the check reads it there, and so does the seed role
    if (kem_hpk_wave(c, n, w.d_pk, (size_t)Dm.pk, Dm.pk, wave)) return -1;
    if (!wave) {
        k_kem_hpk<<<dim3((unsigned)((n + 63) / 64)), dim3(64), 0, c.stream>>>(n, w.d_pk, (size_t)Dm.pk, Dm.pk, nullptr, w.d_h, 32);
        HIPCHK(hipGetLastError());
    }
    RegTreeCheckJob j{};
    j.n = n; j.D = D; j.K = Dm.K; j.slot = c.d_rl_slot; j.h = w.d_h; j.h_stride = 32; j.paths = c.d_rl_rec; j.ok = w.d_mask;
    memcpy(j.root, root, 32);
    HIPCHK(launch_regtree_check(j, c.stream)); // the verdicts are the mask, in HBM
    c.path_n[PATH_REGTREE_CHECK]++;
    HIPCHK(kem_copy_out(c, done, w.d_mask, (size_t)n)); // queued here: the body's last synchronisation covers it
    KemKeySide k = kem_side_items(w, Dm, w.d_pk, (size_t)Dm.pk, false);
    k.h_ready = true;
    return kem_enc_body(c, n, k, coins, ct, ss, w.d_mask, PATH_KEM_ENC_PROVEN);
}

// ---- the registry tree (kosk_registry.hip) ------------------------------------------------------------------
// the slot numbers in w.d_key (copied in, or left there by k_registry_find), k_registry_path into the registry's staging, the copies out
int kem_registry_prove(Ctx &c, int n, const int32_t *slots, const uint8_t *h, uint8_t *hout, int32_t *slots_out, uint8_t *done, uint8_t *paths)
{
    if (n < 1 || n > KEM_CHUNK || (!slots && (!h || !slots_out || !done)) || !c.registry) { c.err = "kem_registry_prove: bad arguments"; return -1; }
    if (kem_ensure(c, n)) return -1;
    if (!slots && registry_index_ensure(c)) return -1;
    if (registry_tree_ensure(c)) return -1;
    if (registry_paths_ensure(c, n)) return -1;
    KemWs &w = *c.kem;
    const KemRegistry &r = *c.registry;
    const int D = regtree::depth(r.capacity);
    if (D > 0 && !paths) { c.err = "kem_registry_prove: bad arguments"; return -1; }
    HIPCHK(hipSetDevice(c.device));
    RegPathJob j{};
    j.n = n; j.D = D; j.slot = w.d_key; j.tree = r.d_tree; j.h = r.d_h; j.paths = r.d_paths;
    if (slots) {
        HIPCHK(hipMemcpyAsync(w.d_key, slots, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, c.stream));
        if (hout) j.hout = w.d_h;
    } else {
        HIPCHK(kem_copy_in(c, w.d_h, h, (size_t)n * 32));
        if (kem_launch_find(c, n, w.d_key, false)) return -1;
        HIPCHK(hipMemsetAsync(w.d_h, 0, (size_t)n * 32, c.stream)); // the staged fingerprints go, as in kem_registry_find
        j.found = w.d_mask;
    }
    HIPCHK(launch_registry_path(j, c.stream));
    c.path_n[PATH_REGISTRY_PATH]++;
    if (D > 0) HIPCHK(kem_copy_out(c, paths, r.d_paths, (size_t)n * D * 32));
    if (slots) {
        if (hout) {
            HIPCHK(kem_copy_out(c, hout, w.d_h, (size_t)n * 32));
            HIPCHK(hipMemsetAsync(w.d_h, 0, (size_t)n * 32, c.stream));
        }
    } else {
        HIPCHK(kem_copy_out(c, slots_out, w.d_key, (size_t)n * sizeof(int32_t)));
        HIPCHK(kem_copy_out(c, done, w.d_mask, (size_t)n));
    }
    HIPCHK(stream_sync(c));
    return slots ? 0 : device_error_check(c); // index overflow
}

} // namespace kosk
