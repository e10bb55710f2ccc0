// Compact wire format of the proof: the reference ships the raw struct image of mpcith_proof
// (mlwe_prover.cpp:540-543, 0.65-0.73 MB), in which every share is a u16 below q = 3329.  The compact form keeps the 24
// fields in the same order and packs each u16 field two values into three bytes (12 bits each, value 2i in the low 12
// bits: byte0 = a & 0xFF, byte1 = (a >> 8) | ((b & 0xF) << 4), byte2 = b >> 4 -- the bit order of Kyber's poly_tobytes,
// poly.c:128-147); the two digest fields stay raw; every field starts on a 16-byte boundary.  Lossless for any image whose
// u16 values are below 4096 (every image an honest prover emits; a larger value makes compression fail, not wrap).
// K=3: 680 980 -> 531 760 bytes (78 %).  Packing runs on the GPU in front of the D2H copy of kosk_fetch_proofs_compact and
// unpacking behind the H2D copy of kosk_stage_verifier_inputs_compact, so PCIe carries the compact bytes.
// The dense wire format (kosk_dense.hip) runs the same two kernels on a second field plan with truncated counts.
#include <hip/hip_runtime.h>

#include <cstring>

#include "kosk_ctx.hpp"

namespace kosk {

#define HIPCHK(x) KOSK_HIPCHK(x)

CompactPlan make_compact_plan(const Params &P)
{
    CompactPlan cp{};
    size_t o = 0;
    for (int f = 0; f < NFIELDS; f++) {
        cp.f[f].src_off = (uint32_t)P.off[f];
        cp.f[f].dst_off = (uint32_t)o;
        cp.f[f].raw = (f == F_TCOMM || f == F_COMM);
        cp.f[f].n = (uint32_t)(cp.f[f].raw ? P.size[f] : P.size[f] / 2); // bytes (raw) or u16 values
        const size_t bytes = cp.f[f].raw ? P.size[f] : P.size[f] / 2 * 3 / 2;
        o += (bytes + 15) / 16 * 16;
    }
    cp.bytes = o;
    return cp;
}

// host codec (same layout), for callers that hold images in host memory
int compact_encode(const Params &P, const uint8_t *img, uint8_t *out)
{
    const CompactPlan cp = make_compact_plan(P);
    memset(out, 0, cp.bytes);
    for (int f = 0; f < NFIELDS; f++) {
        const CompactField &cf = cp.f[f];
        if (cf.raw) { memcpy(out + cf.dst_off, img + cf.src_off, cf.n); continue; }
        const uint8_t *s = img + cf.src_off;
        uint8_t *d = out + cf.dst_off;
        for (uint32_t i = 0; i + 1 < cf.n; i += 2) {
            const uint32_t a = s[2 * i] | (s[2 * i + 1] << 8), b = s[2 * i + 2] | (s[2 * i + 3] << 8);
            if (a >= 4096 || b >= 4096) return -1;
            d[0] = (uint8_t)a; d[1] = (uint8_t)((a >> 8) | ((b & 0xF) << 4)); d[2] = (uint8_t)(b >> 4);
            d += 3;
        }
    }
    return 0;
}
void compact_decode(const Params &P, const uint8_t *in, uint8_t *img)
{
    const CompactPlan cp = make_compact_plan(P);
    for (int f = 0; f < NFIELDS; f++) {
        const CompactField &cf = cp.f[f];
        if (cf.raw) { memcpy(img + cf.src_off, in + cf.dst_off, cf.n); continue; }
        const uint8_t *s = in + cf.dst_off;
        uint8_t *d = img + cf.src_off;
        for (uint32_t i = 0; i + 1 < cf.n; i += 2) {
            const uint32_t a = s[0] | ((s[1] & 0xF) << 8), b = (s[1] >> 4) | (s[2] << 4);
            d[2 * i] = (uint8_t)a; d[2 * i + 1] = (uint8_t)(a >> 8); d[2 * i + 2] = (uint8_t)b; d[2 * i + 3] = (uint8_t)(b >> 8);
            s += 3;
        }
    }
}

// one thread per 8 values (16 image bytes as four aligned u32 -> 12 compact bytes as three aligned u32), or per 16 raw bytes
__global__ __launch_bounds__(256) void k_pack_proofs(const uint8_t *__restrict__ img, size_t image_stride, uint8_t *__restrict__ out,
                                                     size_t out_stride, CompactPlan cp, uint32_t *__restrict__ bad)
{
    const CompactField cf = cp.f[blockIdx.y];
    const uint8_t *s = img + (size_t)blockIdx.z * image_stride + cf.src_off;
    uint8_t *d = out + (size_t)blockIdx.z * out_stride + cf.dst_off;
    const uint32_t units = cf.raw ? (cf.n + 15) / 16 : (cf.n + 7) / 8;
    bool overflow = false;
    for (uint32_t u = blockIdx.x * 256 + threadIdx.x; u < units; u += gridDim.x * 256) {
        if (cf.raw) { // field sizes are multiples of 32
            *reinterpret_cast<uint4 *>(d + 16 * u) = *reinterpret_cast<const uint4 *>(s + 16 * u);
            continue;
        }
        const uint32_t left = cf.n - 8 * u; // values from here on (odd only at the end of a truncated field of the dense plan)
        if (left >= 8) {
            const uint32_t *sw = reinterpret_cast<const uint32_t *>(s + 16 * u);
            const uint32_t w0 = sw[0], w1 = sw[1], w2 = sw[2], w3 = sw[3];
            overflow |= ((w0 | w1 | w2 | w3) & 0xF000F000u) != 0;
            // 8 values a0..a7 of 12 bits -> 96 bits, little-endian bit stream
            const uint32_t a0 = w0 & 0xFFF, a1 = (w0 >> 16) & 0xFFF, a2 = w1 & 0xFFF, a3 = (w1 >> 16) & 0xFFF;
            const uint32_t a4 = w2 & 0xFFF, a5 = (w2 >> 16) & 0xFFF, a6 = w3 & 0xFFF, a7 = (w3 >> 16) & 0xFFF;
            uint32_t *dw = reinterpret_cast<uint32_t *>(d + 12 * u);
            dw[0] = a0 | (a1 << 12) | (a2 << 24);
            dw[1] = (a2 >> 8) | (a3 << 4) | (a4 << 16) | (a5 << 28);
            dw[2] = (a5 >> 4) | (a6 << 8) | (a7 << 20);
        } else {
            for (uint32_t i = 0; i + 1 < left; i += 2) {
                const uint16_t *sv = reinterpret_cast<const uint16_t *>(s + 16 * u) + i;
                const uint32_t a = sv[0], b = sv[1];
                overflow |= (a | b) >= 4096;
                uint8_t *db = d + 12 * u + 3 * (i / 2);
                db[0] = (uint8_t)a; db[1] = (uint8_t)((a >> 8) | ((b & 0xF) << 4)); db[2] = (uint8_t)(b >> 4);
            }
            if (left & 1) { // the last value, packed with one trailing zero value
                const uint32_t a = reinterpret_cast<const uint16_t *>(s + 16 * u)[left - 1];
                overflow |= a >= 4096;
                uint8_t *db = d + 12 * u + 3 * (left / 2);
                db[0] = (uint8_t)a; db[1] = (uint8_t)(a >> 8); db[2] = 0;
            }
        }
    }
    if (overflow) atomicOr(&bad[blockIdx.z], 1u);
}

__global__ __launch_bounds__(256) void k_unpack_proofs(const uint8_t *__restrict__ in, size_t in_stride, uint8_t *__restrict__ img,
                                                       size_t image_stride, CompactPlan cp)
{
    const CompactField cf = cp.f[blockIdx.y];
    const uint8_t *s = in + (size_t)blockIdx.z * in_stride + cf.dst_off;
    uint8_t *d = img + (size_t)blockIdx.z * image_stride + cf.src_off;
    const uint32_t units = cf.raw ? (cf.n + 15) / 16 : (cf.n + 7) / 8;
    for (uint32_t u = blockIdx.x * 256 + threadIdx.x; u < units; u += gridDim.x * 256) {
        if (cf.raw) {
            *reinterpret_cast<uint4 *>(d + 16 * u) = *reinterpret_cast<const uint4 *>(s + 16 * u);
            continue;
        }
        const uint32_t left = cf.n - 8 * u;
        if (left >= 8) {
            const uint32_t *sw = reinterpret_cast<const uint32_t *>(s + 12 * u);
            const uint32_t x0 = sw[0], x1 = sw[1], x2 = sw[2];
            const uint32_t a0 = x0 & 0xFFF, a1 = (x0 >> 12) & 0xFFF, a2 = (x0 >> 24) | ((x1 & 0xF) << 8), a3 = (x1 >> 4) & 0xFFF;
            const uint32_t a4 = (x1 >> 16) & 0xFFF, a5 = (x1 >> 28) | ((x2 & 0xFF) << 4), a6 = (x2 >> 8) & 0xFFF, a7 = x2 >> 20;
            uint32_t *dw = reinterpret_cast<uint32_t *>(d + 16 * u);
            dw[0] = a0 | (a1 << 16); dw[1] = a2 | (a3 << 16); dw[2] = a4 | (a5 << 16); dw[3] = a6 | (a7 << 16);
        } else {
            for (uint32_t i = 0; i + 1 < left; i += 2) {
                const uint8_t *sb = s + 12 * u + 3 * (i / 2);
                uint16_t *dv = reinterpret_cast<uint16_t *>(d + 16 * u) + i;
                dv[0] = (uint16_t)(sb[0] | ((sb[1] & 0xF) << 8));
                dv[1] = (uint16_t)((sb[1] >> 4) | (sb[2] << 4));
            }
            if (left & 1) { // the last value of an odd count; its partner is padding
                const uint8_t *sb = s + 12 * u + 3 * (left / 2);
                reinterpret_cast<uint16_t *>(d + 16 * u)[left - 1] = (uint16_t)(sb[0] | ((sb[1] & 0xF) << 8));
            }
        }
    }
}

size_t format_bytes(const Params &P, int fmt)
{
    return fmt == FMT_IMAGE ? P.proof_bytes : fmt == FMT_COMPACT ? make_compact_plan(P).bytes : fmt_dense(fmt) ? make_dense_plan(P, fmt).bytes : 0;
}

void ensure_plans(Ctx &c)
{
    if (c.cplan.bytes) return;
    c.cplan = make_compact_plan(c.P);
    c.compact_stride = (c.cplan.bytes + 63) / 64 * 64;
    c.dplan = make_dense_plan(c.P); // dense records are shorter and go through the same staging buffers
    c.dense_stride = (c.dplan.bytes + 63) / 64 * 64;
    c.d2plan = make_dense_plan(c.P, FMT_DENSE2);
    c.dense2_stride = (c.d2plan.bytes + 63) / 64 * 64;
}

static int ensure_compact(Ctx &c)
{
    if (c.d_compact) return 0;
    ensure_plans(c);
    // a view keeps its own staging, sized for its own callers' batches (the compact calls are never merged).  Packed proofs and their
    // flags, public
    const int G = Inventory::INVG_COMPACT, HOST = Inventory::INV_HOST;
    auto body = [&]() -> int {
        HIPCHK(c.own("d_compact", &c.d_compact, (size_t)c.own_batch * c.compact_stride, 0, G));
        HIPCHK(c.own("d_compact_bad", &c.d_compact_bad, sizeof(uint32_t) * c.own_batch, 0, G));
        HIPCHK(c.own("h_compact", &c.h_compact, (size_t)c.own_batch * c.compact_stride, HOST, G));
        HIPCHK(c.own("h_compact_bad", &c.h_compact_bad, sizeof(uint32_t) * c.own_batch, HOST, G));
        return 0;
    };
    if (body()) { c.inv.release(G); return -1; } // d_compact is null again: a retry starts from nothing
    return 0;
}

// The two stream-level halves of every packed call, on explicit device pointers (the resident buffers and the transcode workspace alike):
// queued on c.stream, not synchronised; images are c.image_stride apart, records w.stride.
// images -> records: padding bytes are zero; d_bad[b] (zeroed by the caller) is set where image b holds a value >= 4096.  dense: the same
// kernel on the dense plan.  It packs rows 0..406 of the seven low-degree fields and does not look at the rows it drops
static int pack_launch(Ctx &c, int n, const WireFmt &w, const uint8_t *d_img, uint8_t *d_rec, uint32_t *d_bad)
{
    HIPCHK(hipMemsetAsync(d_rec, 0, (size_t)n * w.stride, c.stream));
    hipLaunchKernelGGL(k_pack_proofs, dim3(16, NFIELDS, n), dim3(256), 0, c.stream, d_img, c.image_stride, d_rec, w.stride, *w.plan, d_bad);
    HIPCHK(hipGetLastError());
    return 0;
}
// records -> images.  dense: the dropped rows start as zero and stay so where the opened list is malformed (d_status 1; the verifier
// rejects such an image), and the refill of kosk_dense.hip follows the unpack kernel (needs ensure_dense_ws)
static int unpack_launch(Ctx &c, int n, const WireFmt &w, const uint8_t *d_rec, uint8_t *d_img, uint32_t *d_status)
{
    const Params &P = c.P;
    const CompactPlan &plan = *w.plan;
    if (fmt_dense(w.id))
        for (int f = 0; f < NFIELDS; f++)
            if (!plan.f[f].raw && (size_t)plan.f[f].n * 2 < P.size[f])
                HIPCHK(hipMemset2DAsync(d_img + P.off[f] + (size_t)plan.f[f].n * 2, c.image_stride, 0, P.size[f] - (size_t)plan.f[f].n * 2, n, c.stream));
    hipLaunchKernelGGL(k_unpack_proofs, dim3(16, NFIELDS, n), dim3(256), 0, c.stream, d_rec, w.stride, d_img, c.image_stride, plan);
    HIPCHK(hipGetLastError());
    if (fmt_dense(w.id) && dense_fill_launch(c, n, d_img, c.image_stride, d_status, false, w.id)) return -1;
    return 0;
}

// what the library's own prover left in HBM is a codeword by construction (kosk_dense.hip; the host codec checks, this call does not)
int fetch_proofs_packed(Ctx &c, int n, int fmt, uint8_t *out, bool direct)
{
    if (n < 1 || n > c.own_batch) { c.err = "batch size out of range"; return -1; }
    HIPCHK(hipSetDevice(c.device));
    if (ensure_compact(c)) return -1;
    const WireFmt w = wire_fmt(c, fmt);
    HIPCHK(hipMemsetAsync(c.d_compact_bad, 0, sizeof(uint32_t) * n, c.stream));
    if (pack_launch(c, n, w, c.d_proof, c.d_compact, c.d_compact_bad)) return -1;
    // direct: `out` is page-locked host memory (the caller's own, or locked for this call by kosk_capi.cpp): no staging copy
    if (direct) HIPCHK(hipMemcpy2DAsync(out, w.bytes, c.d_compact, w.stride, w.bytes, n, hipMemcpyDeviceToHost, c.stream));
    else HIPCHK(hipMemcpyAsync(c.h_compact, c.d_compact, (size_t)n * w.stride, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipMemcpyAsync(c.h_compact_bad, c.d_compact_bad, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c.stream));
    HIPCHK(stream_sync(c));
    c.path_n[direct ? PATH_COPY_DIRECT : PATH_COPY_STAGED]++;
    for (int b = 0; b < n; b++)
        if (c.h_compact_bad[b]) { c.err = "a resident proof holds a value >= 4096: not representable in the compact format"; return -1; }
    if (!direct)
        parallel_for(c.pool, n, c.nthreads, [&](int b) { memcpy(out + (size_t)b * w.bytes, c.h_compact + (size_t)b * w.stride, w.bytes); });
    return 0;
}

int stage_verifier_inputs_packed(Ctx &c, int n, int fmt, const uint8_t *in, const uint8_t *pk, bool direct)
{
    if (n < 1 || n > c.own_batch) { c.err = "batch size out of range"; return -1; }
    HIPCHK(hipSetDevice(c.device));
    if (ensure_verify_workspace(c)) return -1;
    if (ensure_compact(c)) return -1;
    if (fmt_dense(fmt) && ensure_dense_ws(c)) return -1;
    const Params &P = c.P;
    const WireFmt w = wire_fmt(c, fmt);
    parallel_for(c.pool, n, c.nthreads, [&](int b) {
        memcpy(c.h_pk + (size_t)b * c.pk_stride, pk + (size_t)b * P.pk_bytes, P.pk_bytes);
        if (!direct) memcpy(c.h_compact + (size_t)b * w.stride, in + (size_t)b * w.bytes, w.bytes);
    });
    c.path_n[direct ? PATH_COPY_DIRECT : PATH_COPY_STAGED]++;
    HIPCHK(hipMemcpyAsync(c.d_pk, c.h_pk, (size_t)n * c.pk_stride, hipMemcpyHostToDevice, c.stream));
    c.note_pk_written(n);
    if (direct) HIPCHK(hipMemcpy2DAsync(c.d_compact, w.stride, in, w.bytes, w.bytes, n, hipMemcpyHostToDevice, c.stream));
    else HIPCHK(hipMemcpyAsync(c.d_compact, c.h_compact, (size_t)n * w.stride, hipMemcpyHostToDevice, c.stream));
    if (unpack_launch(c, n, w, c.d_compact, c.d_proof, c.d_dense_status)) return -1;
    HIPCHK(launch_decode_pk(c.d_pk, c.pk_stride, c.d_t, c.d_A, c.key_stride, P.K, n, c.stream, c.xof_guard()));
    HIPCHK(stream_sync(c));
    if (device_error_check(c)) return -1;
    return 0;
}

// ---- transcoding between the four wire formats (kosk_transcode_batch) ----------------------------------------
// Its own workspace, so that nothing resident moves: own_batch 16-byte-aligned images, the records of either side, two status words per
// proof (the refill's / check's, the pack kernel's overflow flag) and their page-locked mirror.  All public: proofs are
struct TcWs {
    uint8_t *d_img = nullptr, *d_in = nullptr, *d_out = nullptr;
    uint32_t *d_words = nullptr, *h_words = nullptr; // [2][own_batch]: dense status, then overflow
};

void transcode_release(Ctx &c)
{
    TcWs *w = c.tc;
    if (!w) return;
    c.inv.release(Inventory::INVG_TRANSCODE);
    delete w;
    c.tc = nullptr;
}

static int transcode_ensure(Ctx &c)
{
    if (c.tc) return 0;
    ensure_plans(c);
    TcWs *w = new TcWs();
    c.tc = w;
    const size_t N = (size_t)c.own_batch;
    const int G = Inventory::INVG_TRANSCODE;
    auto body = [&]() -> int {
        HIPCHK(c.own("tc.d_img", &w->d_img, N * c.image_stride, 0, G));
        HIPCHK(c.own("tc.d_in", &w->d_in, N * c.compact_stride, 0, G));
        HIPCHK(c.own("tc.d_out", &w->d_out, N * c.compact_stride, 0, G));
        HIPCHK(c.own("tc.d_words", &w->d_words, 2 * N * sizeof(uint32_t), 0, G));
        HIPCHK(c.own("tc.h_words", &w->h_words, 2 * N * sizeof(uint32_t), Inventory::INV_HOST, G));
        return 0;
    };
    if (body()) { transcode_release(c); return -1; }
    return 0;
}

// records whose encoder failed (overflow flag, or with use_st a nonzero dense status) become all zero; stride is a multiple of 16
__global__ __launch_bounds__(256) void k_zero_failed(uint8_t *__restrict__ out, size_t stride, const uint32_t *__restrict__ st,
                                                     const uint32_t *__restrict__ bad, int use_st)
{
    const int b = blockIdx.y;
    if (!(bad[b] | (use_st ? st[b] : 0u))) return; // public: a uniform branch
    uint4 *p = reinterpret_cast<uint4 *>(out + (size_t)b * stride);
    for (size_t i = blockIdx.x * 256 + threadIdx.x; i < stride / 16; i += (size_t)gridDim.x * 256) p[i] = make_uint4(0, 0, 0, 0);
}

// n <= own_batch records `from` -> `to` (FMT_*), in / out host (pageable or page-locked) or device memory of any alignment, status on the
// host: the composition of the host codecs per record (kosk_mi355x.h).  On the context's stream, synchronised
int transcode(Ctx &c, int n, int from, const uint8_t *in, int to, uint8_t *out, int32_t *status)
{
    if (n < 1 || n > c.own_batch) { c.err = "batch size out of range"; return -1; }
    HIPCHK(hipSetDevice(c.device));
    if (transcode_ensure(c)) return -1;
    if ((fmt_dense(from) || fmt_dense(to)) && ensure_dense_ws(c)) return -1;
    TcWs &w = *c.tc;
    uint32_t *d_st = w.d_words, *d_bad = w.d_words + c.own_batch;
    const WireFmt wf = wire_fmt(c, from), wt = wire_fmt(c, to);
    HIPCHK(hipMemsetAsync(w.d_words, 0, 2 * (size_t)c.own_batch * sizeof(uint32_t), c.stream));
    // in
    uint8_t *d_src = from == FMT_IMAGE ? w.d_img : w.d_in;
    HIPCHK(hipMemcpy2DAsync(d_src, wf.stride, in, wf.bytes, wf.bytes, n, is_device_pointer(in) ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, c.stream));
    if (from != FMT_IMAGE && unpack_launch(c, n, wf, w.d_in, w.d_img, d_st)) return -1;
    // out
    const uint8_t *d_dst = w.d_img;
    if (to != FMT_IMAGE) {
        if (fmt_dense(to) && dense_fill_launch(c, n, w.d_img, c.image_stride, d_st, true, to)) return -1; // the codeword check
        if (pack_launch(c, n, wt, w.d_img, w.d_out, d_bad)) return -1;
        hipLaunchKernelGGL(k_zero_failed, dim3(8, n), dim3(256), 0, c.stream, w.d_out, wt.stride, d_st, d_bad, fmt_dense(to) ? 1 : 0);
        HIPCHK(hipGetLastError());
        d_dst = w.d_out;
    }
    HIPCHK(hipMemcpy2DAsync(out, wt.bytes, d_dst, wt.stride, wt.bytes, n, is_device_pointer(out) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c.stream));
    HIPCHK(hipMemcpyAsync(w.h_words, w.d_words, 2 * (size_t)c.own_batch * sizeof(uint32_t), hipMemcpyDeviceToHost, c.stream));
    HIPCHK(stream_sync(c));
    if (device_error_check(c)) return -1;
    const uint32_t *st = w.h_words, *bad = w.h_words + c.own_batch;
    for (int b = 0; b < n; b++) {
        const int32_t dec = fmt_dense(from) ? (int32_t)st[b] : 0; // the decoder's: 1 a malformed I
        const int32_t enc = to == FMT_IMAGE ? 0 : bad[b] ? -1 : (fmt_dense(to) && st[b]) ? -2 : 0;
        status[b] = enc ? enc : dec;
    }
    return 0;
}

} // namespace kosk
