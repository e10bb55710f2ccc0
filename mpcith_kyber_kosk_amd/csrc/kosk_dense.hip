// Dense wire format kosk-dense-v1: the compact format's layout, but the seven fields whose rows are
// evaluations of polynomials of degree <= 406 at the points 256 + party (beta, gamma, t, s+r, e+r and the two eta-gate
// fields of the 1304 unopened parties, ascending) keep only rows 0..406.  Rows 407..1303 are a function of those rows and
// of the opened list I: Lagrange interpolation through the nodes x_j = 256 + rest[j], j < 407.
//
// This file holds the host codec (reference-grade: clarity over speed) and the refill on the GPU, which runs behind the
// unpack kernel of kosk_compact.hip.  Kernel plan (DESIGN.md "Dense wire format"): the per-proof operator in barycentric form,
//   out[i][c] = l_i * sum_j inv(x_i - x_j) * (w_j * y[j][c]),
// k_dense_setup makes rest, the weights w_j and l_i of a proof; k_dense_fill builds the table of the 2907 possible differences'
// inverses and the weighted shares of one column group in LDS and hands both to the Cauchy-product engine it shares with
// k_interp_apply (kosk_cauchy_dev.hpp: operand fragments built in registers, int8-limb MFMA k-steps); its own are the column
// groups, the 64-row staging and the stores.  Every global store is 16 bytes.
// k_dense_check (DESIGN.md "Transcoding between the wire formats") is the same body with the other epilogue: the refilled chunks are
// compared with the image's own instead of stored, which is the representability check of the host codec's pack.
//
// kosk-dense-v2 keeps fewer rows of four fields whose sharing polynomials have public values at
// the 256 packed positions: p = kappa + Z v, Z(x) = prod_{a < 256} (x - a).  The same operator on a smaller node set R (151 for the
// eta-gate fields, 557 for the u fields) with 1 / Z(x_j) folded into w_j and Z(x_i) into l_i; the body is a template over the node
// set (3, 7 or 9 k-steps) and over the affine mode (kappa_c taken off the shares, added back in the epilogue).
#include <hip/hip_runtime.h>

#include <cstring>
#include <type_traits>
#include <vector>

#include "kosk_ctx.hpp"
#include "kosk_cauchy_dev.hpp"

namespace kosk {

#define HIPCHK(x) KOSK_HIPCHK(x)

// the truncated fields of a dense format and the rows each keeps: v1 seven fields at 407; v2 the eta-gate fields at
// 151 (constant sharings: public values at the 256 packed positions) and the two u fields at 557 (zero there)
static const int kDenseFields[9] = {F_BETA, F_GAMMA, F_T, F_SR, F_ER, F_SETA, F_EETA, F_US, F_UE};
constexpr int R_ETA = DEG + 1 - NSEC, R_U = DEG2 + 1 - NSEC; // 151, 557
static int dense_rows(int f, int fmt)
{
    const bool v2 = fmt == FMT_DENSE2;
    switch (f) {
    case F_BETA: case F_GAMMA: case F_T: case F_SR: case F_ER: return XLEN;
    case F_SETA: case F_EETA: return v2 ? R_ETA : XLEN;
    case F_US: case F_UE: return v2 ? R_U : 0;
    default: return 0;
    }
}
static inline uint32_t dense_cols(const Params &P, int f) { return (uint32_t)(P.size[f] / 2 / NREST); }

CompactPlan make_dense_plan(const Params &P, int fmt)
{
    CompactPlan cp{};
    size_t o = 0;
    for (int f = 0; f < NFIELDS; f++) {
        cp.f[f].src_off = (uint32_t)P.off[f];
        cp.f[f].dst_off = (uint32_t)o;
        cp.f[f].raw = (f == F_TCOMM || f == F_COMM);
        if (cp.f[f].raw) cp.f[f].n = (uint32_t)P.size[f];
        else if (dense_rows(f, fmt)) cp.f[f].n = (uint32_t)dense_rows(f, fmt) * dense_cols(P, f);
        else cp.f[f].n = (uint32_t)(P.size[f] / 2);
        const size_t bytes = cp.f[f].raw ? cp.f[f].n : (size_t)(cp.f[f].n + 1) / 2 * 3; // an odd count is packed with one trailing zero value
        o += (bytes + 15) / 16 * 16;
    }
    cp.bytes = o;
    return cp;
}

// ---- host codec ----------------------------------------------------------------------------------------------------
static uint32_t inv_mod_q(uint32_t a)
{
    uint32_t r = 1, b = a % Q;
    for (int e = Q - 2; e; e >>= 1) {
        if (e & 1) r = r * b % Q;
        b = b * b % Q;
    }
    return r;
}

// the dropped rows of the truncated fields from the kept ones and I, in place; 1 (nothing written) for a malformed I.
// A field with R kept rows is interpolated through the nodes x_j = 256 + rest[j], j < R.  R = 407: the polynomial itself.  R = 151 / 557:
// p = kappa + Z v with Z(x) = prod_{a < 256} (x - a), so v = (p - kappa) / Z is interpolated and p rebuilt (kappa_c the public constant
// of column c of an eta field, 0 for a u field)
static int dense_refill_host(const Params &P, uint8_t *img, int fmt)
{
    bool opened[NPARTY] = {false};
    for (int t = 0; t < NOPEN; t++) {
        const uint32_t v = img[P.off[F_I] + 2 * t] | (img[P.off[F_I] + 2 * t + 1] << 8);
        if (v >= (uint32_t)NPARTY || opened[v]) return 1;
        opened[v] = true;
    }
    int rest[NREST], nr = 0;
    for (int p = 0; p < NPARTY; p++)
        if (!opened[p]) rest[nr++] = p;
    std::vector<uint32_t> inv(Q, 0);
    for (int a = 1; a < Q; a++) inv[a] = inv_mod_q((uint32_t)a);
    auto diff = [&](int a, int b) { return (uint32_t)((a - b) % Q + Q) % Q; };
    uint32_t Zx[NREST]; // Z(x_i) = prod_{a < 256} (256 + rest[i] - a), never zero: 256 <= x <= 1709 < q
    for (int i = 0; i < NREST; i++) {
        uint32_t z = 1;
        for (int a = 0; a < NSEC; a++) z = z * (uint32_t)(NSEC + rest[i] - a) % Q;
        Zx[i] = z;
    }
    std::vector<uint32_t> w, L, kap;
    std::vector<uint64_t> acc;
    for (const int R : {XLEN, R_ETA, R_U}) {
        const bool viaZ = R != XLEN;
        bool any = false;
        for (int f : kDenseFields) any |= dense_rows(f, fmt) == R;
        if (!any) continue;
        // barycentric weights w_j = 1 / prod_{m != j} (x_j - x_m), with 1 / Z(x_j) folded in
        w.assign(R, 0);
        for (int j = 0; j < R; j++) {
            uint32_t pr = viaZ ? Zx[j] : 1;
            for (int m = 0; m < R; m++)
                if (m != j) pr = pr * diff(rest[j], rest[m]) % Q;
            w[j] = inv[pr];
        }
        L.assign(R, 0);
        for (int i = R; i < NREST; i++) {
            uint32_t l = viaZ ? Zx[i] : 1; // [Z(x_i)] l(x_i), l(x) = prod_j (x - x_j)
            for (int j = 0; j < R; j++) l = l * diff(rest[i], rest[j]) % Q;
            for (int j = 0; j < R; j++) L[j] = l * w[j] % Q * inv[diff(rest[i], rest[j])] % Q;
            for (int f : kDenseFields) {
                if (dense_rows(f, fmt) != R) continue;
                const uint32_t cols = dense_cols(P, f);
                uint8_t *base = img + P.off[f];
                kap.assign(cols, 0);
                if (f == F_SETA || f == F_EETA)
                    for (uint32_t c = 0; c < cols; c++) kap[c] = viaZ ? (uint32_t)((int)(c % (uint32_t)P.E) - P.eta1 + Q) % Q : 0;
                acc.assign(cols, 0);
                for (int j = 0; j < R; j++) {
                    const uint8_t *row = base + (size_t)j * cols * 2;
                    for (uint32_t c = 0; c < cols; c++) acc[c] += (uint64_t)L[j] * (((uint32_t)(row[2 * c] | (row[2 * c + 1] << 8)) % Q + Q - kap[c]) % Q);
                }
                uint8_t *out = base + (size_t)i * cols * 2;
                for (uint32_t c = 0; c < cols; c++) {
                    const uint32_t v = (uint32_t)((acc[c] + kap[c]) % Q);
                    out[2 * c] = (uint8_t)v; out[2 * c + 1] = (uint8_t)(v >> 8);
                }
            }
        }
    }
    return 0;
}

int dense_decode(const Params &P, const uint8_t *in, uint8_t *img, int fmt)
{
    const CompactPlan dp = make_dense_plan(P, fmt);
    memset(img, 0, P.proof_bytes);
    for (int f = 0; f < NFIELDS; f++) {
        const CompactField &cf = dp.f[f];
        if (cf.raw) { memcpy(img + cf.src_off, in + cf.dst_off, cf.n); continue; }
        const uint8_t *s = in + cf.dst_off;
        uint8_t *d = img + cf.src_off;
        for (uint32_t i = 0; i < cf.n; i += 2) {
            const uint32_t a = s[0] | ((s[1] & 0xF) << 8), b = (s[1] >> 4) | (s[2] << 4);
            d[2 * i] = (uint8_t)a; d[2 * i + 1] = (uint8_t)(a >> 8);
            if (i + 1 < cf.n) { d[2 * i + 2] = (uint8_t)b; d[2 * i + 3] = (uint8_t)(b >> 8); }
            s += 3;
        }
    }
    return dense_refill_host(P, img, fmt);
}

int dense_encode(const Params &P, const uint8_t *img, uint8_t *out, int fmt)
{
    const CompactPlan dp = make_dense_plan(P, fmt);
    memset(out, 0, dp.bytes);
    for (int f = 0; f < NFIELDS; f++) {
        const CompactField &cf = dp.f[f];
        if (cf.raw) { memcpy(out + cf.dst_off, img + cf.src_off, cf.n); continue; }
        const uint8_t *s = img + cf.src_off;
        uint8_t *d = out + cf.dst_off;
        for (uint32_t i = 0; i < cf.n; i += 2) {
            const uint32_t a = s[2 * i] | (s[2 * i + 1] << 8), b = i + 1 < cf.n ? (uint32_t)(s[2 * i + 2] | (s[2 * i + 3] << 8)) : 0u;
            if (a >= 4096 || b >= 4096) return -1;
            d[0] = (uint8_t)a; d[1] = (uint8_t)((a >> 8) | ((b & 0xF) << 4)); d[2] = (uint8_t)(b >> 4);
            d += 3;
        }
    }
    // representable iff the dropped rows are what unpack makes of the kept ones
    std::vector<uint8_t> back(P.proof_bytes);
    if (dense_decode(P, out, back.data(), fmt)) return -2;
    return memcmp(back.data(), img, P.proof_bytes) ? -2 : 0;
}

// ---- the refill on the GPU -----------------------------------------------------------------------------------------
constexpr int DN_KS = 7, DN_NTMAX = 5, DN_MAXF = 5; // 448 node slots; a column group has up to 80 columns of up to 5 fields
constexpr int DN_NGROUPS = 3, DN_NGROUPS2 = 5;      // column groups (workgroups per proof) of v1 / v2
constexpr int DN_TAB = 2 * NPARTY - 1;              // limb pairs of 1/d at index d + NPARTY - 1, |d| <= 1453
// per-proof workspace, u16: rest[1344] (ascending complement of I, zero behind 1304), w[448] (zero behind 407), l[960] (zero behind 897);
// v2's two further node sets behind them: w'[192] (zero behind 151), l'[1216] (zero behind 1153); w'[576] (zero behind 557), l'[768]
// (zero behind 747).  v1 leaves the second half untouched
constexpr int DN_WS_REST = 0, DN_WS_W = 1344, DN_WS_ELL = 1344 + 448, DN_WS_V1 = 1344 + 448 + 960;
constexpr int DN_WS_W_ETA = DN_WS_V1, DN_WS_ELL_ETA = DN_WS_W_ETA + 192, DN_WS_W_U = DN_WS_ELL_ETA + 1216, DN_WS_ELL_U = DN_WS_W_U + 576;
constexpr int DN_WS = DN_WS_ELL_U + 768;            // 5504 u16 per proof
constexpr int DN_STAGE = 128 * NCHK + DN_MAXF * 32; // 64 rows of the widest group + per field a carry chunk and a tail chunk

// A node set: the first R entries of the complement are the nodes, the other 1304 - R the rows to fill
enum { DN_SET_D = 0, DN_SET_ETA = 1, DN_SET_U = 2 };
template <int SET> struct DnSet;
template <> struct DnSet<DN_SET_D> { static constexpr int R = XLEN, WS_W = DN_WS_W, WS_ELL = DN_WS_ELL; static constexpr bool AFFINE = false; };
template <> struct DnSet<DN_SET_ETA> { static constexpr int R = R_ETA, WS_W = DN_WS_W_ETA, WS_ELL = DN_WS_ELL_ETA; static constexpr bool AFFINE = true; };
template <> struct DnSet<DN_SET_U> { static constexpr int R = R_U, WS_W = DN_WS_W_U, WS_ELL = DN_WS_ELL_U; static constexpr bool AFFINE = false; }; // kappa = 0
template <int SET> struct DnDim {
    static constexpr int R = DnSet<SET>::R;
    static constexpr int KS = (R + 63) / 64;       // 7 / 3 / 9 k-steps; the slots behind R hold zero weights
    static constexpr int NTGT = NREST - R;         // 897 / 1153 / 747 rows to fill
    static constexpr int ITERS = (NTGT + 63) / 64; // 15 / 19 / 12 passes of 64 rows (4 waves x 16); the last one holds 1 / 1 / 43 rows
    static constexpr int ELLN = ITERS * 64;
};
static_assert(DnDim<DN_SET_D>::KS == DN_KS && DnDim<DN_SET_D>::ELLN == 960 && DnDim<DN_SET_ETA>::ELLN == 1216 && DnDim<DN_SET_U>::ELLN == 768, "workspace layout");
static_assert(DnDim<DN_SET_U>::KS * 2 <= DN_KS * DN_NTMAX && DnDim<DN_SET_ETA>::KS * 3 <= DN_KS * DN_NTMAX, "v2's tiles fit the v1 share buffer");
constexpr int DN_ELL_MAX = DnDim<DN_SET_ETA>::ELLN;

struct DenseFillField { uint32_t start, cols, col0; }; // image offset of the first dropped row of the field, columns per row, first column in the group
struct DenseFillGroup { int nf, ncols, set, E; DenseFillField f[DN_MAXF]; }; // set: DN_SET_*; E = 2 eta1 + 1 (kappa of an eta column)
template <int NG> struct DenseFillArgsT { DenseFillGroup g[NG]; }; // a launch argument: v1 carries its three groups only
using DenseFillArgs = DenseFillArgsT<DN_NGROUPS>;
using DenseFill2Args = DenseFillArgsT<DN_NGROUPS2>;

// opened list -> status, rest, w, l of one proof; grid (6, n): block x owns entries [256 x, 256 x + 256) of the complement.
// V2: also the weights of the node sets R = 151 and R = 557, from the same running product and Z(x_r) = prod_{t = 1..256} (rest[r] + t)
template <bool V2>
__device__ __forceinline__ void dense_setup(const uint8_t *__restrict__ img, size_t image_stride, uint32_t off_I,
                                            uint16_t *__restrict__ ws, uint32_t *__restrict__ status)
{
    __shared__ int mark_s[NPARTY];
    __shared__ int cnt_s[256];
    __shared__ uint16_t rest_s[NREST + 8];
    __shared__ int bad_s;
    const int tid = threadIdx.x, b = blockIdx.y;
    for (int p = tid; p < NPARTY; p += 256) mark_s[p] = 0;
    if (tid == 0) bad_s = 0;
    __syncthreads();
    if (tid < NOPEN) {
        const uint32_t v = *reinterpret_cast<const uint16_t *>(img + (size_t)b * image_stride + off_I + 2 * tid);
        if (v >= (uint32_t)NPARTY) atomicOr(&bad_s, 1);
        else if (atomicAdd(&mark_s[v], 1) != 0) atomicOr(&bad_s, 1);
    }
    __syncthreads();
    if (bad_s) { // I is public: a uniform branch
        if (blockIdx.x == 0 && tid == 0) status[b] = 1;
        return;
    }
    constexpr int PER = (NPARTY + 255) / 256; // 6 parties per thread
    const int p0 = tid * PER, p1 = min(p0 + PER, NPARTY);
    int cnt = 0;
    for (int p = p0; p < p1; p++) cnt += mark_s[p] == 0;
    cnt_s[tid] = cnt;
    __syncthreads();
    int base = 0;
    for (int t = 0; t < tid; t++) base += cnt_s[t];
    for (int p = p0; p < p1; p++)
        if (mark_s[p] == 0) rest_s[base++] = (uint16_t)p;
    __syncthreads();
    uint16_t *wsb = ws + (size_t)b * DN_WS;
    if (blockIdx.x == 0) {
        if (tid == 0) status[b] = 0;
        for (int r = tid; r < DN_WS_W; r += 256) wsb[DN_WS_REST + r] = r < NREST ? rest_s[r] : (uint16_t)0;
    }
    const int r = blockIdx.x * 256 + tid;
    if (r < NREST) {
        const int xr = rest_s[r];
        uint32_t pr = 1, pr_eta = 1;
        for (int m = 0; m < XLEN; m++) {
            if (V2 && m == R_ETA) pr_eta = pr;
            const uint32_t d = gf_diff(xr - (int)rest_s[m]);
            pr = gf_mul_fast(pr, m == r ? 1u : d);
        }
        if (r < XLEN) wsb[DN_WS_W + r] = (uint16_t)gf_inv_pow(pr); // w_j = 1 / prod_{m != j} (x_j - x_m)
        else wsb[DN_WS_ELL + r - XLEN] = (uint16_t)pr;          // l(x_i) = prod_j (x_i - x_j)
        if constexpr (V2) {
            for (int m = XLEN; m < R_U; m++) {
                const uint32_t d = gf_diff(xr - (int)rest_s[m]);
                pr = gf_mul_fast(pr, m == r ? 1u : d);
            }
            uint32_t z = 1; // Z(256 + p) = (p + 1) ... (p + 256): every factor is below q
            for (int t = 1; t <= NSEC; t++) z = gf_mul_fast(z, (uint32_t)(xr + t));
            const uint32_t p_eta = gf_mul_fast(z, pr_eta), p_u = gf_mul_fast(z, pr);
            if (r < R_ETA) wsb[DN_WS_W_ETA + r] = (uint16_t)gf_inv_pow(p_eta); // w'_j = 1 / (Z(x_j) prod_{m != j} (x_j - x_m))
            else wsb[DN_WS_ELL_ETA + r - R_ETA] = (uint16_t)p_eta;          // l'_i = Z(x_i) prod_j (x_i - x_j)
            if (r < R_U) wsb[DN_WS_W_U + r] = (uint16_t)gf_inv_pow(p_u);
            else wsb[DN_WS_ELL_U + r - R_U] = (uint16_t)p_u;
        }
    } else {
        const int z = r - NREST; // the padding both vectors need, written by the last block's idle threads
        if (z < 448 - XLEN) wsb[DN_WS_W + XLEN + z] = 0;
        else if (z - (448 - XLEN) < 960 - (NREST - XLEN)) wsb[DN_WS_ELL + (NREST - XLEN) + z - (448 - XLEN)] = 0;
    }
    if (V2 && blockIdx.x == 0) { // the padding of the two further node sets
        if (tid < 192 - R_ETA) wsb[DN_WS_W_ETA + R_ETA + tid] = 0;
        if (tid < DnDim<DN_SET_ETA>::ELLN - DnDim<DN_SET_ETA>::NTGT) wsb[DN_WS_ELL_ETA + DnDim<DN_SET_ETA>::NTGT + tid] = 0;
        if (tid < 576 - R_U) wsb[DN_WS_W_U + R_U + tid] = 0;
        if (tid < DnDim<DN_SET_U>::ELLN - DnDim<DN_SET_U>::NTGT) wsb[DN_WS_ELL_U + DnDim<DN_SET_U>::NTGT + tid] = 0;
    }
}
__global__ __launch_bounds__(256) void k_dense_setup(const uint8_t *__restrict__ img, size_t image_stride, uint32_t off_I,
                                                     uint16_t *__restrict__ ws, uint32_t *__restrict__ status)
{
    dense_setup<false>(img, image_stride, off_I, ws, status);
}
__global__ __launch_bounds__(256) void k_dense2_setup(const uint8_t *__restrict__ img, size_t image_stride, uint32_t off_I,
                                                      uint16_t *__restrict__ ws, uint32_t *__restrict__ status)
{
    dense_setup<true>(img, image_stride, off_I, ws, status);
}

// the weighted shares of this workgroup's column group, read from LDS where the MFMAs use them
struct DenseFragsLds {
    const uint8_t *y_s;
    int NT, lane;
    __device__ __forceinline__ void ahead(int) {}
    __device__ __forceinline__ v4i frag(int ks, int j, int limb) const { return *reinterpret_cast<const v4i *>(y_s + frag_offset(16 * j, 64 * ks, limb, NT) + 16 * lane); }
};

// One workgroup per (column group, proof).  The rows a field gains are one contiguous byte range of the image; the workgroup
// walks it 64 rows at a time through an LDS buffer per field and writes it out in aligned 16-byte chunks, carrying the
// bytes behind the last whole chunk to the next pass.  The first chunk is completed with the kept bytes in front of the range
// and the last one with the bytes behind it (the next field's kept rows), both read from the image and written back as they
// are: no other workgroup writes those bytes.
// CHECK (k_dense_check, the codeword check of kosk_transcode_batch): the same product with the other epilogue.  Where the fill stores a
// chunk the check loads it from the image and compares; any difference ends as bit 1 of the proof's status word.  The carry and tail
// bytes come from the image in both, so they compare equal and only a filled row can differ.  The image is read only.
template <bool CHECK> using dense_img_t = std::conditional_t<CHECK, const uint8_t, uint8_t>;
template <bool CHECK> using dense_status_t = std::conditional_t<CHECK, uint32_t, const uint32_t>;

// SET: the node set (DnSet / DnDim).  An affine set's shares arrive with kappa_c taken off (dense_fill_group) and get it back here
template <int SET, int NT, bool CHECK>
__device__ __forceinline__ void dense_fill_body(dense_img_t<CHECK> *__restrict__ imgb, const DenseFillGroup &g, const uint16_t *tab_s, const uint16_t *rest_s,
                                                const uint16_t *ell_s, const uint8_t *y_s, uint8_t *stage_s, const uint32_t *cstart_s,
                                                const uint16_t *ccols_s, const uint16_t *ccf_s, const uint16_t *csb_s, const uint16_t *ckap_s,
                                                dense_status_t<CHECK> *status_b)
{
    constexpr int R = DnDim<SET>::R, KS = DnDim<SET>::KS, NTGT = DnDim<SET>::NTGT, ITERS = DnDim<SET>::ITERS;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    uint32_t differs = 0; // CHECK: OR of image chunk ^ recomputed chunk over this thread's chunks
    uint16_t *stage16 = reinterpret_cast<uint16_t *>(stage_s);
#pragma unroll 1
    for (int it = 0; it < ITERS; it++) {
        const int m0 = it * 64 + wv * 16;
        if (m0 < NTGT) { // uniform per wave
            const int ri = min(R + m0 + (lane & 15), NREST - 1); // rows behind 1303 repeat the last one and are not stored
            const int kq = (int)rest_s[ri] + NPARTY - 1;
            DenseFragsLds ld{y_s, NT, lane};
            CauchySums<KS, NT> cs;
            cs.template run<0>(rest_s, tab_s, lane, kq, ld); // kq - x_j in [0, 2906]: both are parties below 1454 (the status word)
            // D[row = target m0 + 4 (lane >> 4) + r][col = column 16 j + (lane & 15)]
            const int lr = wv * 16 + (lane >> 4) * 4, tr = it * 64 + lr; // row of this pass, target
#pragma unroll
            for (int j = 0; j < NT; j++) {
                const int col = j * 16 + (lane & 15);
                const uint32_t cols = ccols_s[col];
                if (cols == 0) continue; // padding column
                const uint32_t carry = (cstart_s[col] + (uint32_t)it * 128u * cols) & 15u;
                const uint32_t at = (uint32_t)csb_s[col] + carry + 2u * ccf_s[col];
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    if (tr + r >= NTGT) continue;
                    uint32_t v = gf_mul_fast(ell_s[tr + r], cs.value(j, r));
                    if constexpr (DnSet<SET>::AFFINE) {
                        v += ckap_s[col];
                        v = min(v, v - (uint32_t)Q);
                    }
                    stage16[(at + (uint32_t)(lr + r) * cols * 2u) >> 1] = (uint16_t)v;
                }
            }
        }
        // the tail chunk of the last pass is completed with the image's bytes behind the range
        const int rows = min(64, NTGT - it * 64);
        uint32_t keep[DN_MAXF];
#pragma unroll
        for (int f = 0; f < DN_MAXF; f++) {
            keep[f] = 0;
            if (f >= g.nf) continue;
            const uint32_t cols = g.f[f].cols, pos = g.f[f].start + (uint32_t)it * 128u * cols, carry = pos & 15u;
            const uint32_t total = carry + (uint32_t)rows * cols * 2u, sb = csb_s[g.f[f].col0];
            if (it == ITERS - 1 && (total & 15u) && tid < 8 && total + 2u * tid < ((total + 15u) & ~15u))
                stage16[(sb + total) / 2 + tid] = *reinterpret_cast<const uint16_t *>(imgb + (pos - carry) + total + 2 * tid);
        }
        __syncthreads();
#pragma unroll
        for (int f = 0; f < DN_MAXF; f++) {
            if (f >= g.nf) continue;
            const uint32_t cols = g.f[f].cols, pos = g.f[f].start + (uint32_t)it * 128u * cols, carry = pos & 15u;
            const uint32_t total = carry + (uint32_t)rows * cols * 2u, sb = csb_s[g.f[f].col0];
            const uint32_t nfull = it == ITERS - 1 ? (total + 15u) >> 4 : total >> 4;
            for (uint32_t k = tid; k < nfull; k += 256) {
                const uint4 mine = *reinterpret_cast<const uint4 *>(stage_s + sb + 16 * k);
                if constexpr (CHECK) {
                    const uint4 theirs = *reinterpret_cast<const uint4 *>(imgb + (pos - carry) + 16 * k);
                    differs |= (mine.x ^ theirs.x) | (mine.y ^ theirs.y) | (mine.z ^ theirs.z) | (mine.w ^ theirs.w);
                } else {
                    *reinterpret_cast<uint4 *>(imgb + (pos - carry) + 16 * k) = mine;
                }
            }
            // the bytes behind the last whole chunk (bit 16: this thread's pair is one of them)
            if (2u * tid < (total & 15u) && it < ITERS - 1) keep[f] = stage16[(sb + 16 * nfull) / 2 + tid] | 0x10000u;
        }
        __syncthreads();
        if (tid < 8) {
#pragma unroll
            for (int f = 0; f < DN_MAXF; f++)
                if (f < g.nf && (keep[f] >> 16)) stage16[csb_s[g.f[f].col0] / 2 + tid] = (uint16_t)keep[f];
        }
        // the next pass writes behind its carry, i.e. behind these bytes; its flush comes after the next barrier
    }
    if constexpr (CHECK)
        if (differs) atomicOr(status_b, 2u); // images are public, and so is what the check says about them
}

// One column group on node set SET, behind the column tables: the weighted shares and the carry bytes into LDS, then the body at the
// group's tile count.  The tile counts are those that occur: v1 70 | 70 | 34 / 39 / 52 columns, v2 70 | 70 | 6 / 9 / 12 on the 407 nodes,
// 28 / 30 / 40 eta columns on 151, 24 / 24 / 32 u columns on 557
template <int SET, bool CHECK, bool V2>
__device__ __forceinline__ void dense_fill_group(dense_img_t<CHECK> *__restrict__ imgb, const DenseFillGroup &g, const uint16_t *__restrict__ wsb,
                                                 const uint16_t *tab_s, const uint16_t *rest_s, uint16_t *ell_s, uint8_t *y_s, uint8_t *stage_s,
                                                 const uint32_t *cstart_s, const uint16_t *ccols_s, const uint16_t *ccf_s, const uint16_t *csb_s,
                                                 const uint16_t *ckap_s, dense_status_t<CHECK> *status_b)
{
    constexpr int R = DnDim<SET>::R, KS = DnDim<SET>::KS, WS_W = DnSet<SET>::WS_W;
    const int tid = threadIdx.x, nt = (g.ncols + 15) >> 4;
    // weighted shares w_j (y[j][c] mod q [- kappa_c]) of this group's columns: one thread per (column, 16 nodes), consecutive threads on consecutive columns
    const int ncp = nt * 16;
    for (int t = tid; t < ncp * KS * 4; t += 256) {
        const int c = t % ncp, kc16 = t / ncp;
        const uint32_t cols = ccols_s[c];
        cauchy_weighted_frag(y_s, c, kc16, nt, cols != 0, [&](uint32_t (&y)[16], uint32_t (&w)[16]) {
            const uint8_t *src = imgb + (cstart_s[c] - (uint32_t)R * cols * 2u) + 2u * ccf_s[c]; // row 0 of the field, this column
            const uint32_t off = DnSet<SET>::AFFINE ? (uint32_t)Q - ckap_s[c] : 0u;
#pragma unroll
            for (int q = 0; q < 16; q++) {
                const int j = kc16 * 16 + q;
                w[q] = wsb[WS_W + j]; // zero behind the nodes (k_dense_setup)
                const uint32_t v = j < R ? *reinterpret_cast<const uint16_t *>(src + (size_t)j * cols * 2) : 0u;
                y[q] = DnSet<SET>::AFFINE ? gf_reduce_u32(v) + off : v; // below 2 q; a slot behind the nodes has weight 0
            }
        });
    }
    // the bytes between the 16-byte boundary and the first filled row: kept rows, read back from the image
    if (tid < 8)
        for (int f = 0; f < g.nf; f++) {
            const uint32_t carry = g.f[f].start & 15u;
            if (2u * tid < carry)
                reinterpret_cast<uint16_t *>(stage_s)[csb_s[g.f[f].col0] / 2 + tid] = *reinterpret_cast<const uint16_t *>(imgb + (g.f[f].start - carry) + 2 * tid);
        }
    __syncthreads();
#define DN_BODY(NT) dense_fill_body<SET, NT, CHECK>(imgb, g, tab_s, rest_s, ell_s, y_s, stage_s, cstart_s, ccols_s, ccf_s, csb_s, ckap_s, status_b)
    if constexpr (SET == DN_SET_D && !V2) {
        if (nt == 5) DN_BODY(5);
        else if (nt == 4) DN_BODY(4);
        else DN_BODY(3);
    } else if constexpr (SET == DN_SET_D) {
        if (nt == 5) DN_BODY(5);
        else DN_BODY(1);
    } else if constexpr (SET == DN_SET_ETA) {
        if (nt == 3) DN_BODY(3);
        else DN_BODY(2);
    } else {
        DN_BODY(2);
    }
#undef DN_BODY
}

template <bool CHECK, bool V2>
__device__ __forceinline__ void dense_fill_kernel(dense_img_t<CHECK> *__restrict__ img, size_t image_stride, const DenseFillArgsT<V2 ? DN_NGROUPS2 : DN_NGROUPS> &A,
                                                  const uint16_t *__restrict__ ws, dense_status_t<CHECK> *__restrict__ status)
{
    __shared__ __attribute__((aligned(16))) uint8_t y_s[DN_KS * DN_NTMAX * 2048];
    __shared__ __attribute__((aligned(16))) uint8_t stage_s[DN_STAGE];
    __shared__ __attribute__((aligned(16))) uint16_t rest_s[DN_WS_W];
    __shared__ __attribute__((aligned(4))) uint16_t tab_s[DN_TAB + 1];
    __shared__ uint16_t ell_s[V2 ? DN_ELL_MAX : 960];
    __shared__ uint32_t cstart_s[DN_NTMAX * 16];
    __shared__ uint16_t ccols_s[DN_NTMAX * 16], ccf_s[DN_NTMAX * 16], csb_s[DN_NTMAX * 16], ckap_s[DN_NTMAX * 16];
    const int tid = threadIdx.x, b = blockIdx.y;
    // malformed opened list: nothing is written (the check looks at bit 0 only: bit 1 is its own, set by a workgroup that is done)
    if (CHECK ? (status[b] & 1u) != 0 : status[b] != 0) return;
    const DenseFillGroup &g = A.g[blockIdx.x];
    dense_img_t<CHECK> *imgb = img + (size_t)b * image_stride;
    const uint16_t *wsb = ws + (size_t)b * DN_WS;

    for (int i = tid; i < DN_TAB; i += 256) tab_s[i] = limb_pair(gf_inv_pow(gf_diff(i - (NPARTY - 1)))); // 1/d, d = i - 1453 (0 for d = 0: met only by zero shares)
    for (int i = tid; i < DN_WS_W; i += 256) rest_s[i] = wsb[DN_WS_REST + i];
    { // l_i of the group's node set (v1: constants)
        const bool d = !V2 || g.set == DN_SET_D, eta = g.set == DN_SET_ETA;
        const int off = d ? DnSet<DN_SET_D>::WS_ELL : eta ? DnSet<DN_SET_ETA>::WS_ELL : DnSet<DN_SET_U>::WS_ELL;
        const int cnt = d ? DnDim<DN_SET_D>::ELLN : eta ? DnDim<DN_SET_ETA>::ELLN : DnDim<DN_SET_U>::ELLN;
        for (int i = tid; i < cnt; i += 256) ell_s[i] = wsb[off + i];
    }
    if (tid < DN_NTMAX * 16) { // column -> field, column in the field, the field's LDS buffer
        uint32_t start = 0, cols = 0, cf = 0, sb = 0, o = 0;
        for (int f = 0; f < g.nf; f++) {
            if ((uint32_t)tid >= g.f[f].col0 && (uint32_t)tid < g.f[f].col0 + g.f[f].cols) { start = g.f[f].start; cols = g.f[f].cols; cf = tid - g.f[f].col0; sb = o; }
            o += 128 * g.f[f].cols + 32;
        }
        cstart_s[tid] = start; ccols_s[tid] = (uint16_t)cols; ccf_s[tid] = (uint16_t)cf; csb_s[tid] = (uint16_t)sb;
        // kappa_c = (c mod (2 eta1 + 1)) - eta1 mod q: what column c of an eta-gate field shares at all 256 packed positions
        if constexpr (V2) ckap_s[tid] = (uint16_t)((cf % (uint32_t)g.E + (uint32_t)Q - (uint32_t)(g.E >> 1)) % (uint32_t)Q);
    }
    __syncthreads();
    if constexpr (!V2) {
        dense_fill_group<DN_SET_D, CHECK, false>(imgb, g, wsb, tab_s, rest_s, ell_s, y_s, stage_s, cstart_s, ccols_s, ccf_s, csb_s, ckap_s, status + b);
    } else { // the group's node set is a launch argument: uniform
        if (g.set == DN_SET_D) dense_fill_group<DN_SET_D, CHECK, true>(imgb, g, wsb, tab_s, rest_s, ell_s, y_s, stage_s, cstart_s, ccols_s, ccf_s, csb_s, ckap_s, status + b);
        else if (g.set == DN_SET_ETA) dense_fill_group<DN_SET_ETA, CHECK, true>(imgb, g, wsb, tab_s, rest_s, ell_s, y_s, stage_s, cstart_s, ccols_s, ccf_s, csb_s, ckap_s, status + b);
        else dense_fill_group<DN_SET_U, CHECK, true>(imgb, g, wsb, tab_s, rest_s, ell_s, y_s, stage_s, cstart_s, ccols_s, ccf_s, csb_s, ckap_s, status + b);
    }
}

__global__ __launch_bounds__(256) void k_dense_fill(uint8_t *__restrict__ img, size_t image_stride, DenseFillArgs A, const uint16_t *__restrict__ ws,
                                                    const uint32_t *__restrict__ status)
{
    dense_fill_kernel<false, false>(img, image_stride, A, ws, status);
}
// d_status[b]: 0, 1 (k_dense_setup: malformed I) or 2 (a u16 of rows 407..1303 of a listed field is not the refill of rows 0..406)
__global__ __launch_bounds__(256) void k_dense_check(const uint8_t *__restrict__ img, size_t image_stride, DenseFillArgs A, const uint16_t *__restrict__ ws,
                                                     uint32_t *__restrict__ status)
{
    dense_fill_kernel<true, false>(img, image_stride, A, ws, status);
}
// kosk-dense-v2: five column groups per proof (grid (5, n)) behind k_dense2_setup; the status words as above, on v2's dropped rows
__global__ __launch_bounds__(256) void k_dense2_fill(uint8_t *__restrict__ img, size_t image_stride, DenseFill2Args A, const uint16_t *__restrict__ ws,
                                                     const uint32_t *__restrict__ status)
{
    dense_fill_kernel<false, true>(img, image_stride, A, ws, status);
}
__global__ __launch_bounds__(256) void k_dense2_check(const uint8_t *__restrict__ img, size_t image_stride, DenseFill2Args A, const uint16_t *__restrict__ ws,
                                                      uint32_t *__restrict__ status)
{
    dense_fill_kernel<true, true>(img, image_stride, A, ws, status);
}

// the groups of format `fmt`: three for v1, five for v2
static DenseFill2Args make_fill_args(const Params &P, int fmt)
{
    DenseFill2Args a{};
    auto put = [&](DenseFillGroup &g, int f) {
        DenseFillField &d = g.f[g.nf++];
        d.cols = dense_cols(P, f);
        d.start = (uint32_t)(P.off[f] + (size_t)dense_rows(f, fmt) * d.cols * 2);
        d.col0 = (uint32_t)g.ncols;
        g.ncols += (int)d.cols;
    };
    for (DenseFillGroup &g : a.g) { g.set = DN_SET_D; g.E = P.E; }
    put(a.g[0], F_BETA);
    put(a.g[1], F_GAMMA);
    if (fmt == FMT_DENSE) {
        for (int f : {F_T, F_SR, F_ER, F_SETA, F_EETA}) put(a.g[2], f); // 34 / 39 / 52 columns (K = 2 / 3 / 4)
    } else {
        for (int f : {F_T, F_SR, F_ER}) put(a.g[2], f); // 6 / 9 / 12 columns
        a.g[3].set = DN_SET_ETA;
        for (int f : {F_SETA, F_EETA}) put(a.g[3], f);  // 28 / 30 / 40 columns on 151 nodes
        a.g[4].set = DN_SET_U;
        for (int f : {F_US, F_UE}) put(a.g[4], f);      // 24 / 24 / 32 columns on 557 nodes
    }
    return a;
}

int ensure_dense_ws(Ctx &c)
{
    if (c.d_dense_ws) return 0;
    // rows of proof images and a status word per proof, public
    auto body = [&]() -> int {
        HIPCHK(c.own("d_dense_ws", &c.d_dense_ws, (size_t)c.own_batch * DN_WS * sizeof(uint16_t), 0, Inventory::INVG_DENSE));
        HIPCHK(c.own("d_dense_status", &c.d_dense_status, sizeof(uint32_t) * c.own_batch, 0, Inventory::INVG_DENSE));
        return 0;
    };
    if (body()) { c.inv.release(Inventory::INVG_DENSE); return -1; }
    return 0;
}

// the dropped rows of format `fmt` (FMT_DENSE: rows 407..1303 of the seven fields; FMT_DENSE2: of its nine fields from their own first
// dropped row) of n <= own_batch images in HBM, in place, on the context's stream (no synchronisation);
// check: compared with what is there instead of stored (d_status 0 / 1 / 2, the images are only read)
int dense_fill_launch(Ctx &c, int n, uint8_t *d_images, size_t image_stride, uint32_t *d_status, bool check, int fmt)
{
    const bool v2 = fmt == FMT_DENSE2;
    if (n < 1 || n > c.own_batch) { c.err = "batch size out of range"; return -1; }
    if ((reinterpret_cast<uintptr_t>(d_images) | image_stride) & 15) {
        c.err = std::string(v2 ? "dense2 " : "dense ") + (check ? "check" : "fill") + ": images and their stride must be 16-byte aligned";
        return -1;
    }
    if (image_stride < c.P.proof_bytes) {
        c.err = std::string(v2 ? "dense2 " : "dense ") + (check ? "check" : "fill") + ": image stride below kosk_proof_bytes";
        return -1;
    }
    if (ensure_dense_ws(c)) return -1;
    const DenseFill2Args a = make_fill_args(c.P, fmt);
    DenseFillArgs a1{};
    for (int i = 0; i < DN_NGROUPS; i++) a1.g[i] = a.g[i];
    const dim3 sgrid(6, n), grid(v2 ? DN_NGROUPS2 : DN_NGROUPS, n);
    if (v2) hipLaunchKernelGGL(k_dense2_setup, sgrid, dim3(256), 0, c.stream, d_images, image_stride, (uint32_t)c.P.off[F_I], c.d_dense_ws, d_status);
    else hipLaunchKernelGGL(k_dense_setup, sgrid, dim3(256), 0, c.stream, d_images, image_stride, (uint32_t)c.P.off[F_I], c.d_dense_ws, d_status);
    HIPCHK(hipGetLastError());
    if (v2 && check) hipLaunchKernelGGL(k_dense2_check, grid, dim3(256), 0, c.stream, d_images, image_stride, a, c.d_dense_ws, d_status);
    else if (v2) hipLaunchKernelGGL(k_dense2_fill, grid, dim3(256), 0, c.stream, d_images, image_stride, a, c.d_dense_ws, d_status);
    else if (check) hipLaunchKernelGGL(k_dense_check, grid, dim3(256), 0, c.stream, d_images, image_stride, a1, c.d_dense_ws, d_status);
    else hipLaunchKernelGGL(k_dense_fill, grid, dim3(256), 0, c.stream, d_images, image_stride, a1, c.d_dense_ws, d_status);
    HIPCHK(hipGetLastError());
    c.path_n[v2 ? (check ? PATH_DENSE2_CHECK : PATH_DENSE2_FILL) : (check ? PATH_DENSE_CHECK : PATH_DENSE_FILL)]++;
    return 0;
}

int dense_fill_device(Ctx &c, int n, uint8_t *d_images, size_t image_stride, uint32_t *d_status, bool check, int fmt)
{
    HIPCHK(hipSetDevice(c.device));
    for (int done = 0; done < n;) {
        const int m = n - done < c.own_batch ? n - done : c.own_batch;
        if (dense_fill_launch(c, m, d_images + (size_t)done * image_stride, image_stride, d_status + done, check, fmt)) return -1;
        done += m;
    }
    HIPCHK(stream_sync(c));
    if (device_error_check(c)) return -1;
    return 0;
}

} // namespace kosk
