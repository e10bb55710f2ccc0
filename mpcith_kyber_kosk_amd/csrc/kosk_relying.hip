// The relying party: proofs of the two state trees checked in batches against ONE root, that of a signed
// head.  What the registrar's kernels build (kosk_registry.hip, kosk_regsort.hip) a peer hands over with its key; these kernels walk it back.
//   k_regtree_check   one lane per item: the leaf (L(h) or E), then `depth` nodes up the path, four words against the root, one byte out
//   k_regsort_check   a lane pair per item, the left walk on the even lane and the right walk on the odd one, joined by a shuffle; the
//                     decision is regsort::check_decide, the code the host function runs
// One sponge per lane (kosk_keccak_dev.hpp, perm), the states those of kosk_regtree.hpp / kosk_regsort.hpp.  Everything here is public peer
// data: branches and addresses may depend on it.  The loop bound `depth` is grid-uniform; what a lane finds wrong with its item (a slot
// outside the tree, a position outside it, a negative slot in a key leaf) only selects its verdict: the lane finishes the walk on a clamped
// index, and no branch goes around perm.
#include <hip/hip_runtime.h>

#include <cstring>

#include "kosk_ctx.hpp"
#include "kosk_kem_dev.hpp"
#include "kosk_regsort.hpp"

namespace kosk {

using namespace kem;

#define HIPCHK(x) KOSK_HIPCHK(x)

__device__ __forceinline__ void words_load16(const uint8_t *src, uint64_t (&d)[4]) // 16-byte aligned
{
    const U128 a = reinterpret_cast<const U128 *>(src)[0], b = reinterpret_cast<const U128 *>(src)[1];
    d[0] = (uint64_t)a.x | (uint64_t)a.y << 32; d[1] = (uint64_t)a.z | (uint64_t)a.w << 32;
    d[2] = (uint64_t)b.x | (uint64_t)b.y << 32; d[3] = (uint64_t)b.z | (uint64_t)b.w << 32;
}

// `depth` steps from the digest in st[0..3]: step l is N(sib, cur) where bit l of pos is set, else N(cur, sib).  NODE: the format's node_state
template <class NODE> __device__ __forceinline__ void walk_up(uint64_t (&st)[25], int D, uint32_t pos, const uint8_t *path, NODE &&node)
{
    for (int l = 0; l < D; l++) {
        uint64_t sib[4], a[4], b[4];
        words_load16(path + (size_t)l * 32, sib);
        const bool odd = (pos >> l) & 1;
#pragma unroll
        for (int w = 0; w < 4; w++) { a[w] = odd ? sib[w] : st[w]; b[w] = odd ? st[w] : sib[w]; }
        node(st, a, b);
        perm(st);
    }
}

__device__ __forceinline__ bool words_equal(const uint64_t (&st)[25], const uint64_t (&r)[4])
{
    return ((st[0] ^ r[0]) | (st[1] ^ r[1]) | (st[2] ^ r[2]) | (st[3] ^ r[3])) == 0;
}

__global__ __launch_bounds__(64) void k_regtree_check(RegTreeCheckJob j)
{
    const long b = (long)blockIdx.x * 64 + threadIdx.x;
    if (b >= j.n) return;
    const int32_t slot = j.slot[b];
    const bool occupied = !j.state || j.state[b] != 0;
    bool good = slot >= 0 && ((uint32_t)slot >> j.D) == 0 && !(occupied && !j.h);
    const uint32_t pos = slot >= 0 && ((uint32_t)slot >> j.D) == 0 ? (uint32_t)slot : 0u;
    uint64_t st[25];
    if (occupied && j.h) {
        uint64_t h[4];
#pragma unroll
        for (int l = 0; l < 4; l++) h[l] = ld64(j.h + (size_t)b * j.h_stride, l);
        regtree::leaf_state(st, j.K, h);
    } else {
        regtree::empty_state(st, j.K);
    }
    perm(st);
    walk_up(st, j.D, pos, j.paths + (size_t)b * j.D * 32, [](uint64_t (&s)[25], const uint64_t (&l)[4], const uint64_t (&r)[4]) { regtree::node_state(s, l, r); });
    good = good && words_equal(st, j.root);
    j.ok[b] = good ? 1 : 0;
}

// a against b as 32 bytes in memcmp order (16-byte aligned): < 0, 0, > 0
__device__ __forceinline__ int cmp32(const uint8_t *a, const uint8_t *b)
{
    uint64_t x[4], y[4];
    words_load16(a, x);
    words_load16(b, y);
    int r = 0;
#pragma unroll
    for (int l = 3; l >= 0; l--) {
        const uint64_t u = __builtin_bswap64(x[l]), v = __builtin_bswap64(y[l]);
        if (u != v) r = u < v ? -1 : 1;
    }
    return r;
}

// Lanes 2 i and 2 i + 1 of a wave take item i of the block (32 items a block): side 0 walks (pos_l, S(h_l, slot_l), path_l), side 1 walks
// (pos_l + 1, S(h_r, slot_r) or Z by bit2 of flags, path_r) -- whatever the flags say of the side's presence: an absent side's half is walked
// and its result is never asked for.  walked = what regsort::root_from_path + memcmp give: the position inside the tree, no negative slot in
// a key leaf, the digest equal to root.  A pair behind the last item repeats the last item and writes nothing: every lane reaches the shuffle
__global__ __launch_bounds__(64) void k_regsort_check(RegSortCheckJob j)
{
    const long pair = (long)blockIdx.x * 32 + (threadIdx.x >> 1);
    const int side = threadIdx.x & 1;
    const bool live = pair < j.n;
    const size_t b = (size_t)(live ? pair : j.n - 1);
    const size_t rec_bytes = regsort::proof_bytes(j.D);
    const uint8_t *rec = j.rec + b * rec_bytes, *x = j.x + b * 32;
    const U128 head = *reinterpret_cast<const U128 *>(rec);
    const int64_t pos_l = (int32_t)head.x;
    const uint32_t flags = head.w;
    const bool leaf_key = side == 0 || (flags & regsort::FLAG_RIGHT_KEY);
    const int32_t slot = (int32_t)(side == 0 ? head.y : head.z);
    const int64_t at = pos_l + side;
    const bool inside = at >= 0 && (at >> j.D) == 0;
    uint64_t st[25];
    if (leaf_key) {
        uint64_t h[4];
        words_load16(rec + (side == 0 ? regsort::REC_H_L : regsort::REC_H_R), h);
        regsort::leaf_state(st, j.K, h, (uint32_t)slot);
    } else {
        regsort::pad_state(st, j.K);
    }
    perm(st);
    walk_up(st, j.D, inside ? (uint32_t)at : 0u, rec + regsort::REC_PATHS + (size_t)side * j.D * 32,
            [](uint64_t (&s)[25], const uint64_t (&l)[4], const uint64_t (&r)[4]) { regsort::node_state(s, l, r); });
    const int walked = inside && !(leaf_key && slot < 0) && words_equal(st, j.root) ? 1 : 0;
    const int other = __shfl_xor(walked, 1);
    const int walk_l = side == 0 ? walked : other, walk_r = side == 0 ? other : walked;
    const int verdict = regsort::check_decide(j.D, pos_l, flags, cmp32(rec + regsort::REC_H_L, x), cmp32(x, rec + regsort::REC_H_R),
                                              [&] { return walk_l != 0; }, [&] { return walk_r != 0; });
    if (live && side == 0) j.verdict[b] = (uint8_t)verdict;
}

hipError_t launch_regtree_check(const RegTreeCheckJob &j, hipStream_t st)
{
    k_regtree_check<<<dim3((unsigned)((j.n + 63) / 64)), dim3(64), 0, st>>>(j);
    return hipGetLastError();
}

hipError_t launch_regsort_check(const RegSortCheckJob &j, hipStream_t st)
{
    k_regsort_check<<<dim3((unsigned)((j.n + 31) / 32)), dim3(64), 0, st>>>(j);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------------------------- host --
int relying_ensure(Ctx &c, int n, size_t rec_bytes)
{
    if (n <= c.rl_cap && rec_bytes <= c.rl_rec) return 0;
    HIPCHK(hipSetDevice(c.device));
    const int G = Inventory::INVG_RELYING;
    if (c.rl_cap) {
        HIPCHK(stream_sync(c));
        c.inv.release(G);
        (void)hipGetLastError();
    }
    const int want = n > c.rl_cap ? n : c.rl_cap;
    const size_t N = (size_t)((want + 1023) / 1024 * 1024 < KEM_CHUNK ? (want + 1023) / 1024 * 1024 : KEM_CHUNK);
    const size_t rec = rec_bytes > c.rl_rec ? rec_bytes : c.rl_rec;
    c.rl_cap = 0;
    c.rl_rec = 0;
    // public, all five: what a peer sent, and what anyone computes from it and a public root
    if (c.own("relying.d_rec", &c.d_rl_rec, N * rec + 16, 0, G) != hipSuccess || c.own("relying.d_q", &c.d_rl_q, N * 32, 0, G) != hipSuccess ||
        c.own("relying.d_state", &c.d_rl_state, N, 0, G) != hipSuccess || c.own("relying.d_ok", &c.d_rl_ok, N, 0, G) != hipSuccess ||
        c.own("relying.d_slot", &c.d_rl_slot, N * sizeof(int32_t), 0, G) != hipSuccess) {
        c.inv.release(G);
        (void)hipGetLastError();
        c.err = "relying_ensure: out of memory for the staging buffers";
        return -1;
    }
    c.rl_cap = (int)N;
    c.rl_rec = rec;
    return 0;
}

static hipError_t copy_in(Ctx &c, void *d_dst, const void *src, size_t bytes)
{
    return hipMemcpyAsync(d_dst, src, bytes, is_device_pointer(src) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c.stream);
}
static hipError_t copy_out(Ctx &c, void *dst, const void *d_src, size_t bytes)
{
    return hipMemcpyAsync(dst, d_src, bytes, is_device_pointer(dst) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c.stream);
}

int regtree_check_paths(Ctx &c, int n, int D, const int32_t *slots, const uint8_t *state, const uint8_t *h, const uint8_t *paths, const uint8_t *root, uint8_t *ok)
{
    if (n < 1 || n > KEM_CHUNK || D < 0 || D > 31 || !slots || (!state && !h) || (D > 0 && !paths) || !root || !ok) { c.err = "regtree_check_paths: bad arguments"; return -1; }
    if (relying_ensure(c, n, (size_t)D * 32)) return -1;
    HIPCHK(hipSetDevice(c.device));
    RegTreeCheckJob j{};
    j.n = n; j.D = D; j.K = c.P.K; j.slot = c.d_rl_slot; j.paths = c.d_rl_rec; j.ok = c.d_rl_ok;
    memcpy(j.root, root, 32);
    HIPCHK(copy_in(c, c.d_rl_slot, slots, (size_t)n * sizeof(int32_t)));
    if (state) { HIPCHK(copy_in(c, c.d_rl_state, state, (size_t)n)); j.state = c.d_rl_state; }
    if (h) { HIPCHK(copy_in(c, c.d_rl_q, h, (size_t)n * 32)); j.h = c.d_rl_q; j.h_stride = 32; }
    if (D > 0) HIPCHK(copy_in(c, c.d_rl_rec, paths, (size_t)n * D * 32));
    HIPCHK(launch_regtree_check(j, c.stream));
    c.path_n[PATH_REGTREE_CHECK]++;
    HIPCHK(copy_out(c, ok, c.d_rl_ok, (size_t)n));
    HIPCHK(stream_sync(c));
    return 0;
}

int regsort_check_proofs(Ctx &c, int n, int D, const uint8_t *x, const uint8_t *records, const uint8_t *root, uint8_t *verdict)
{
    if (n < 1 || n > KEM_CHUNK || D < 0 || D > 31 || !x || !records || !root || !verdict) { c.err = "regsort_check_proofs: bad arguments"; return -1; }
    const size_t rec = regsort::proof_bytes(D);
    if (relying_ensure(c, n, rec)) return -1;
    HIPCHK(hipSetDevice(c.device));
    RegSortCheckJob j{};
    j.n = n; j.D = D; j.K = c.P.K; j.x = c.d_rl_q; j.rec = c.d_rl_rec; j.verdict = c.d_rl_ok;
    memcpy(j.root, root, 32);
    HIPCHK(copy_in(c, c.d_rl_q, x, (size_t)n * 32));
    HIPCHK(copy_in(c, c.d_rl_rec, records, (size_t)n * rec));
    HIPCHK(launch_regsort_check(j, c.stream));
    c.path_n[PATH_REGSORT_CHECK]++;
    HIPCHK(copy_out(c, verdict, c.d_rl_ok, (size_t)n));
    HIPCHK(stream_sync(c));
    return 0;
}

} // namespace kosk
