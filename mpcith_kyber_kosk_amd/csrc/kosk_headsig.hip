// Signed heads (kosk-headsig-v1, kosk_headsig.hpp): the registrar's hash-based signature over a history head.
//   leaves   k_headsig_leaves   a lane per (leaf, chain), 7 leaves a block: x_q[i] from the seed, 255 chain steps in registers, the 34 ends
//                               through LDS, one lane per leaf absorbs the nine blocks of K_q and hashes T[2^h + q]
//   tree     k_headsig_tree     one tier: 1 024 nodes through 10 levels in LDS a block.  A sibling of k_registry_tree, not that kernel with a
//                               functor: a node hashes its own number, so the block needs the heap numbering, and the tree has no empty
//                               leaves, no dirty list and no wave tail
//   sign     k_headsig_sign     one block: S from the root where k_reghist_frontier left it, C, Q, 34 chains of a[i] steps, the path gathered
//   verify   k_headsig_verify   the chain engine from z[i] at step a[i], K', the leaf, h nodes up the path, four words against T[1]
// One sponge per lane (kosk_keccak_dev.hpp through kem::perm).  Secrets: the seed is read, never branched or indexed on; x and every chain
// value below a[i] live in registers; the chain ends (public) pass through LDS, which the block zeroes before it ends.  Chain lengths depend
// on Q, which is public; the bounds of every loop around a barrier are block-uniform.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>

#include "kosk_ctx.hpp"
#include "kosk_headsig.hpp"
#include "kosk_kem_dev.hpp"
#include "kosk_reghist.hpp"

namespace kosk {

using namespace kem;

#define HIPCHK(x) KOSK_HIPCHK(x)

__device__ __forceinline__ void hs_load(const uint8_t *src, uint64_t (&d)[4]) // 16-byte aligned
{
    const U128 a = reinterpret_cast<const U128 *>(src)[0], b = reinterpret_cast<const U128 *>(src)[1];
    d[0] = (uint64_t)a.x | (uint64_t)a.y << 32; d[1] = (uint64_t)a.z | (uint64_t)a.w << 32;
    d[2] = (uint64_t)b.x | (uint64_t)b.y << 32; d[3] = (uint64_t)b.z | (uint64_t)b.w << 32;
}
__device__ __forceinline__ void hs_store(uint8_t *dst, const uint64_t (&d)[4]) // 16-byte aligned
{
    reinterpret_cast<U128 *>(dst)[0] = U128{(uint32_t)d[0], (uint32_t)(d[0] >> 32), (uint32_t)d[1], (uint32_t)(d[1] >> 32)};
    reinterpret_cast<U128 *>(dst)[1] = U128{(uint32_t)d[2], (uint32_t)(d[2] >> 32), (uint32_t)d[3], (uint32_t)(d[3] >> 32)};
}
__device__ __forceinline__ void hs_digest(uint64_t (&s)[25], uint64_t (&out)[4])
{
    perm(s);
#pragma unroll
    for (int l = 0; l < 4; l++) out[l] = s[l];
}
// the chain engine: t through steps from .. 254 of chain i of leaf q, the state in registers
__device__ __forceinline__ void hs_chain(const headsig::Id &id, uint32_t q, uint32_t i, int from, int to, uint64_t (&t)[4])
{
    const uint64_t head = headsig::head6(q, i);
    uint64_t s[25];
#pragma unroll 1
    for (int j = from; j < to; j++) {
        headsig::chain_state(s, id, head, (uint32_t)j, t);
        hs_digest(s, t);
    }
}
// the one lane of an item: T[2^h + q] from the item's 34 chain ends in LDS
__device__ __forceinline__ void hs_leaf(const headsig::Id &id, int h, uint32_t q, const uint64_t *Y, uint64_t (&out)[4])
{
    uint64_t s[25], k[4];
    headsig::ots_public_state(s, id, q, [&](int l) { return Y[l]; });
    hs_digest(s, k);
    headsig::leaf_state(s, id, ((uint32_t)1 << h) + q, k);
    hs_digest(s, out);
}
__device__ __forceinline__ void hs_lds_clear(uint64_t *Y, int tid)
{
    __syncthreads();
    for (int l = tid; l < headsig::ITEMS_PER_BLOCK * headsig::Y_WORDS; l += headsig::BLOCK_THREADS) Y[l] = 0;
}

// Lane tid is chain tid % 34 of item tid / 34; lanes 238 .. 255 only keep the barriers.  An item behind the last repeats the last and
// writes nothing.
__global__ __launch_bounds__(headsig::BLOCK_THREADS) void k_headsig_leaves(HeadSigLeavesJob j)
{
    __shared__ __align__(16) uint64_t Y[headsig::ITEMS_PER_BLOCK * headsig::Y_WORDS];
    const int tid = threadIdx.x, it = tid / headsig::CHAINS, ch = tid - it * headsig::CHAINS;
    const bool active = it < headsig::ITEMS_PER_BLOCK;
    const uint32_t item = blockIdx.x * headsig::ITEMS_PER_BLOCK + (uint32_t)it;
    const bool live = active && item < j.count;
    const uint32_t q = j.first + (item < j.count ? item : j.count - 1);
    const headsig::Id id{{j.id[0], j.id[1]}};
    if (active) {
        uint64_t seed[4], s[25], t[4];
#pragma unroll
        for (int l = 0; l < 4; l++) seed[l] = ld64(j.seed, l);
        headsig::chain_state(s, id, headsig::head6(q, (uint32_t)ch), headsig::TAG_X, seed);
        hs_digest(s, t);
        hs_chain(id, q, (uint32_t)ch, 0, headsig::STEPS, t);
#pragma unroll
        for (int l = 0; l < 4; l++) Y[it * headsig::Y_WORDS + 4 * ch + l] = t[l];
    }
    __syncthreads();
    if (active && ch == 0) {
        uint64_t leaf[4];
        hs_leaf(id, j.h, q, Y + it * headsig::Y_WORDS, leaf);
        if (live) hs_store(j.out ? j.out + (size_t)item * 32 : j.tree + ((((size_t)1 << j.h) + q) << 5), leaf);
    }
    hs_lds_clear(Y, tid);
}

// Block b of tier t: the nodes numbered 2^rem + 1 024 b .. of the level rem = h - 10 t below the root, then the levels above them, each node
// written to the tree and kept in LDS for the next level.  Two regions, ping-pong: a level never reads what it writes
__global__ __launch_bounds__(256) void k_headsig_tree(HeadSigTreeJob j)
{
    __shared__ __align__(16) uint64_t A[headsig::TIER_INPUTS * 4];
    __shared__ __align__(16) uint64_t B[headsig::TIER_INPUTS * 2];
    const int tid = threadIdx.x;
    const int rem = j.h - headsig::TIER_LEVELS * j.tier; // >= 1
    const uint32_t in_total = (uint32_t)1 << rem;
    const uint32_t cnt = in_total < (uint32_t)headsig::TIER_INPUTS ? in_total : (uint32_t)headsig::TIER_INPUTS;
    const uint32_t in_base = in_total + blockIdx.x * (uint32_t)headsig::TIER_INPUTS;
    const headsig::Id id{{j.id[0], j.id[1]}};
    for (uint32_t i = tid; i < cnt; i += 256) {
        uint64_t d[4];
        hs_load(j.tree + ((size_t)(in_base + i) << 5), d);
#pragma unroll
        for (int l = 0; l < 4; l++) A[4 * i + l] = d[l];
    }
    __syncthreads();
    const int levels = rem < headsig::TIER_LEVELS ? rem : (int)headsig::TIER_LEVELS;
    for (int lv = 1; lv <= levels; lv++) {
        const uint64_t *in = (lv & 1) ? A : B;
        uint64_t *out = (lv & 1) ? B : A;
        const uint32_t n_out = cnt >> lv, base = (in_total >> lv) + blockIdx.x * ((uint32_t)headsig::TIER_INPUTS >> lv);
        for (uint32_t i = tid; i < n_out; i += 256) {
            uint64_t l4[4], r4[4], s[25], d[4];
#pragma unroll
            for (int l = 0; l < 4; l++) { l4[l] = in[8 * i + l]; r4[l] = in[8 * i + 4 + l]; }
            headsig::node_state(s, id, base + i, l4, r4);
            hs_digest(s, d);
            hs_store(j.tree + ((size_t)(base + i) << 5), d);
#pragma unroll
            for (int l = 0; l < 4; l++) out[4 * i + l] = d[l];
        }
        __syncthreads();
    }
}

// Lanes 0 .. 33: chain `lane` from x_q[lane] through a[lane] steps (a[] comes from Q, which is public); lanes 34 .. 34 + h - 1: the path's
// nodes; lane 63: the signed root behind the record.  No LDS, no barrier
__global__ __launch_bounds__(64) void k_headsig_sign(HeadSigSignJob j)
{
    const int lane = threadIdx.x;
    const uint32_t q = j.size;
    const headsig::Id id{{j.id[0], j.id[1]}};
    uint64_t root[4];
#pragma unroll
    for (int l = 0; l < 4; l++) root[l] = j.root ? ld64(j.root, l) : j.root_imm[l];
    if (lane < headsig::CHAINS) {
        uint64_t seed[4], s[25], c[4], Q[4], t[4];
#pragma unroll
        for (int l = 0; l < 4; l++) seed[l] = ld64(j.seed, l);
        headsig::chain_state(s, id, headsig::head6(q, headsig::TAG_C), headsig::TAG_X, seed);
        hs_digest(s, c);
        headsig::digest_state(s, id, q, c, root, q, j.K);
        hs_digest(s, Q);
        const int a = (int)headsig::coefficient(Q, lane);
        headsig::chain_state(s, id, headsig::head6(q, (uint32_t)lane), headsig::TAG_X, seed);
        hs_digest(s, t);
        hs_chain(id, q, (uint32_t)lane, 0, a, t);
        hs_store(j.sig + headsig::SIG_Z + 32 * lane, t);
        if (lane == 0) {
            *reinterpret_cast<U128 *>(j.sig) = U128{(uint32_t)j.h, q, 0, 0};
            hs_store(j.sig + headsig::SIG_C, c);
        }
    } else if (lane - headsig::CHAINS < j.h) {
        const int l = lane - headsig::CHAINS;
        const size_t r = ((((size_t)1 << j.h) + q) >> l) ^ 1;
        uint64_t d[4];
        hs_load(j.tree + (r << 5), d);
        hs_store(j.sig + headsig::SIG_PATH + 32 * l, d);
    } else if (lane == 63) {
        hs_store(j.sig + headsig::sig_bytes(j.h), root);
    }
}

// What the header check finds wrong with an item only selects its verdict: the lanes finish the walk on leaf 0
__global__ __launch_bounds__(headsig::BLOCK_THREADS) void k_headsig_verify(HeadSigVerifyJob j)
{
    __shared__ __align__(16) uint64_t Y[headsig::ITEMS_PER_BLOCK * headsig::Y_WORDS];
    const int tid = threadIdx.x, it = tid / headsig::CHAINS, ch = tid - it * headsig::CHAINS;
    const bool active = it < headsig::ITEMS_PER_BLOCK;
    const long item = (long)blockIdx.x * headsig::ITEMS_PER_BLOCK + it;
    const bool live = active && item < j.n;
    const size_t b = (size_t)(item < j.n ? item : j.n - 1);
    const uint8_t *sig = j.sigs + b * j.sig_bytes;
    const int32_t size = j.sizes[b];
    const U128 head = *reinterpret_cast<const U128 *>(sig);
    const bool good = head.x == (uint32_t)j.h && size >= 0 && head.y == (uint32_t)size && ((uint32_t)size >> j.h) == 0 && !head.z && !head.w;
    const uint32_t q = good ? (uint32_t)size : 0u;
    const headsig::Id id{{j.id[0], j.id[1]}};
    if (active) {
        uint64_t s[25], c[4], root[4], Q[4], t[4];
        hs_load(sig + headsig::SIG_C, c);
        hs_load(j.roots + b * 32, root);
        headsig::digest_state(s, id, q, c, root, q, j.K);
        hs_digest(s, Q);
        hs_load(sig + headsig::SIG_Z + 32 * ch, t);
        hs_chain(id, q, (uint32_t)ch, (int)headsig::coefficient(Q, ch), headsig::STEPS, t);
#pragma unroll
        for (int l = 0; l < 4; l++) Y[it * headsig::Y_WORDS + 4 * ch + l] = t[l];
    }
    __syncthreads();
    if (active && ch == 0) {
        uint64_t cur[4], s[25];
        hs_leaf(id, j.h, q, Y + it * headsig::Y_WORDS, cur);
        uint32_t number = ((uint32_t)1 << j.h) + q;
        for (int l = 0; l < j.h; l++) {
            uint64_t sib[4], x[4], y[4];
            hs_load(sig + headsig::SIG_PATH + 32 * l, sib);
            const bool odd = number & 1;
#pragma unroll
            for (int w = 0; w < 4; w++) { x[w] = odd ? sib[w] : cur[w]; y[w] = odd ? cur[w] : sib[w]; }
            number >>= 1;
            headsig::node_state(s, id, number, x, y);
            hs_digest(s, cur);
        }
        const bool same = ((cur[0] ^ j.top[0]) | (cur[1] ^ j.top[1]) | (cur[2] ^ j.top[2]) | (cur[3] ^ j.top[3])) == 0;
        if (live) j.ok[b] = good && same ? 1 : 0;
    }
    hs_lds_clear(Y, tid);
}

// ---------------------------------------------------------------------------------------------------------------- host --
static hipError_t copy_in(Ctx &c, void *d_dst, const void *src, size_t bytes)
{
    return hipMemcpyAsync(d_dst, src, bytes, is_device_pointer(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c.stream);
}
static hipError_t copy_out(Ctx &c, void *dst, const void *d_src, size_t bytes)
{
    return hipMemcpyAsync(dst, d_src, bytes, is_device_pointer(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c.stream);
}
// KOSK_DEBUG_HEADSIG_LEAF_LAUNCH: a lower bound for the tests, so that the multi-launch path runs on a small tree
static uint32_t leaf_launch_max()
{
    const char *e = getenv("KOSK_DEBUG_HEADSIG_LEAF_LAUNCH");
    const int v = e ? atoi(e) : 0;
    return v >= 1 && v < (int)headsig::LEAF_LAUNCH_MAX ? (uint32_t)v : (uint32_t)headsig::LEAF_LAUNCH_MAX;
}
static int launch_leaves(Ctx &c, HeadSigLeavesJob j)
{
    k_headsig_leaves<<<dim3((j.count + headsig::ITEMS_PER_BLOCK - 1) / headsig::ITEMS_PER_BLOCK), dim3(headsig::BLOCK_THREADS), 0, c.stream>>>(j);
    HIPCHK(hipGetLastError());
    c.path_n[PATH_HEADSIG_LEAVES]++;
    return 0;
}

void headsig_note_wiped(Ctx &c) { c.sg_has_seed = false; }

void headsig_signer_release(Ctx &c)
{
    if (!c.sg_height) return;
    if (c.d_sg_seed) { // the seed does not go back to the allocator readable
        (void)hipMemsetAsync(c.d_sg_seed, 0, 64, c.stream);
        (void)hipStreamSynchronize(c.stream);
    }
    c.inv.release(Inventory::INVG_SIGNER);
    (void)hipGetLastError();
    c.sg_height = 0;
    c.sg_has_seed = false;
    memset(c.sg_pub, 0, sizeof c.sg_pub);
}

int headsig_signer_reserve(Ctx &c, int height, const uint8_t *seed, const uint8_t *id, uint8_t *pub)
{
    HIPCHK(hipSetDevice(c.device));
    if (!height) {
        HIPCHK(stream_sync(c));
        headsig_signer_release(c);
        return 0;
    }
    uint8_t idh[16];
    if (is_device_pointer(id)) HIPCHK(hipMemcpy(idh, id, 16, hipMemcpyDeviceToHost));
    else memcpy(idh, id, 16);
    HeadSigLeavesJob lj{};
    lj.h = height;
    memcpy(lj.id, idh, 16);
    bool standing = false;
    if (c.sg_height == height && !memcmp(c.sg_pub + headsig::PUB_I, idh, 16)) {
        // the same key identifier over a standing tree: leaf 0 from this seed against T[2^h] decides whether it is the same key
        // (a collision aside, that is "the root matches": the root is a function of the leaves).  The candidate waits in the second half
        // of the secret entry and replaces the resident seed only once it is confirmed: an error on the way leaves the signer as it was
        uint8_t *cand = c.d_sg_seed + 32;
        auto probe = [&]() -> int {
            uint8_t got[32], have[32];
            HIPCHK(copy_in(c, cand, seed, 32));
            lj.seed = cand; lj.first = 0; lj.count = 1; lj.out = c.d_sg_sig;
            if (launch_leaves(c, lj)) return -1;
            HIPCHK(hipMemcpyAsync(got, c.d_sg_sig, 32, hipMemcpyDeviceToHost, c.stream));
            HIPCHK(hipMemcpyAsync(have, c.d_sg_tree + ((size_t)32 << height), 32, hipMemcpyDeviceToHost, c.stream));
            HIPCHK(stream_sync(c));
            standing = !memcmp(got, have, 32);
            if (standing) HIPCHK(hipMemcpyAsync(c.d_sg_seed, cand, 32, hipMemcpyDeviceToDevice, c.stream));
            HIPCHK(hipMemsetAsync(cand, 0, 32, c.stream));
            HIPCHK(stream_sync(c));
            return 0;
        };
        if (probe()) {
            const std::string why = c.err;
            (void)hipMemsetAsync(cand, 0, 32, c.stream);
            (void)hipStreamSynchronize(c.stream);
            (void)hipGetLastError();
            c.err = why;
            return -1;
        }
    }
    if (!standing) {
        HIPCHK(stream_sync(c));
        headsig_signer_release(c);
        const int G = Inventory::INVG_SIGNER; // the tree and the staged signature are public; the seed is the one secret
        if (c.own("signer.d_tree", &c.d_sg_tree, headsig::tree_bytes(height), 0, G) != hipSuccess ||
            c.own("signer.d_sig", &c.d_sg_sig, headsig::sig_bytes(height) + 32, 0, G) != hipSuccess ||
            c.own("signer.d_seed", &c.d_sg_seed, 64, Inventory::INV_SECRET, G) != hipSuccess) {
            c.inv.release(G);
            (void)hipGetLastError();
            c.err = "kosk_registry_signer_reserve: out of memory for the tree";
            return -1;
        }
        c.sg_height = height;
        auto body = [&]() -> int {
            HIPCHK(hipMemsetAsync(c.d_sg_tree, 0, 32, c.stream)); // slot 0 is no node
            HIPCHK(hipMemsetAsync(c.d_sg_seed, 0, 64, c.stream));
            HIPCHK(copy_in(c, c.d_sg_seed, seed, 32));
            lj.seed = c.d_sg_seed; lj.tree = c.d_sg_tree; lj.out = nullptr;
            const uint32_t total = (uint32_t)1 << height, step = leaf_launch_max();
            for (uint32_t first = 0; first < total; first += step) { // many launches on the stream, none of them long
                lj.first = first;
                lj.count = total - first < step ? total - first : step;
                if (launch_leaves(c, lj)) return -1;
            }
            HeadSigTreeJob tj{};
            tj.h = height; tj.tree = c.d_sg_tree;
            memcpy(tj.id, idh, 16);
            for (int t = 0; t * headsig::TIER_LEVELS < height; t++) {
                const int rem = height - t * headsig::TIER_LEVELS;
                tj.tier = t;
                k_headsig_tree<<<dim3(rem <= headsig::TIER_LEVELS ? 1u : 1u << (rem - headsig::TIER_LEVELS)), dim3(256), 0, c.stream>>>(tj);
                HIPCHK(hipGetLastError());
                c.path_n[PATH_HEADSIG_TREE]++;
            }
            headsig::le32_out(c.sg_pub, (uint32_t)height);
            memcpy(c.sg_pub + headsig::PUB_I, idh, 16);
            HIPCHK(hipMemcpyAsync(c.sg_pub + headsig::PUB_ROOT, c.d_sg_tree + 32, 32, hipMemcpyDeviceToHost, c.stream));
            HIPCHK(stream_sync(c));
            return 0;
        };
        if (body()) {
            const std::string why = c.err;
            (void)hipStreamSynchronize(c.stream);
            headsig_signer_release(c);
            c.err = why;
            return -1;
        }
    }
    c.sg_has_seed = true;
    if (is_device_pointer(pub)) HIPCHK(hipMemcpy(pub, c.sg_pub, headsig::PUB_BYTES, hipMemcpyHostToDevice));
    else memcpy(pub, c.sg_pub, headsig::PUB_BYTES);
    return 0;
}

int headsig_sign_head(Ctx &c, int size, uint8_t *sig, uint8_t *root)
{
    KemRegistry &r = *c.registry;
    HIPCHK(hipSetDevice(c.device));
    HeadSigSignJob j{};
    j.h = c.sg_height; j.K = c.P.K; j.size = (uint32_t)size; j.seed = c.d_sg_seed; j.tree = c.d_sg_tree; j.sig = c.d_sg_sig;
    memcpy(j.id, c.sg_pub + headsig::PUB_I, 16);
    if (!size) { // the empty history's head is a constant of kyber_k
        uint8_t o[32];
        (void)reghist::empty_root(c.P.K, o);
        memcpy(j.root_imm, o, 32);
    } else {
        if (reghist_frontier_ensure(c, r, size)) return -1;
        int top = 0;
        while ((size >> top) > 1) top++;
        j.root = r.d_hrag + (size_t)(top + 1) * 32; // read where k_reghist_frontier left it
    }
    k_headsig_sign<<<dim3(1), dim3(64), 0, c.stream>>>(j);
    HIPCHK(hipGetLastError());
    c.path_n[PATH_HEADSIG_SIGN]++;
    const size_t sb = headsig::sig_bytes(c.sg_height);
    HIPCHK(copy_out(c, sig, c.d_sg_sig, sb));
    if (root) HIPCHK(copy_out(c, root, c.d_sg_sig + sb, 32));
    HIPCHK(stream_sync(c));
    return 0;
}

int headsig_verify_heads(Ctx &c, int n, const uint8_t *pub, const uint8_t *roots, const int32_t *sizes, const uint8_t *sigs, uint8_t *ok)
{
    const int h = (int)headsig::le32_in(pub);
    const size_t sb = headsig::sig_bytes(h);
    if (n < 1 || n > KEM_CHUNK || !sb || !roots || !sizes || !sigs || !ok) { c.err = "headsig_verify_heads: bad arguments"; return -1; }
    if (relying_ensure(c, n, sb)) return -1;
    HIPCHK(hipSetDevice(c.device));
    HeadSigVerifyJob j{};
    j.n = n; j.h = h; j.K = c.P.K; j.roots = c.d_rl_q; j.sigs = c.d_rl_rec; j.sizes = c.d_rl_slot; j.sig_bytes = sb; j.ok = c.d_rl_ok;
    memcpy(j.id, pub + headsig::PUB_I, 16);
    memcpy(j.top, pub + headsig::PUB_ROOT, 32);
    HIPCHK(copy_in(c, c.d_rl_q, roots, (size_t)n * 32));
    HIPCHK(copy_in(c, c.d_rl_slot, sizes, (size_t)n * sizeof(int32_t)));
    HIPCHK(copy_in(c, c.d_rl_rec, sigs, (size_t)n * sb));
    k_headsig_verify<<<dim3((unsigned)((n + headsig::ITEMS_PER_BLOCK - 1) / headsig::ITEMS_PER_BLOCK)), dim3(headsig::BLOCK_THREADS), 0, c.stream>>>(j);
    HIPCHK(hipGetLastError());
    c.path_n[PATH_HEADSIG_VERIFY]++;
    HIPCHK(copy_out(c, ok, c.d_rl_ok, (size_t)n));
    HIPCHK(stream_sync(c));
    return 0;
}

} // namespace kosk
