// Witness recovery from an existing Kyber secret key for kosk_witness_kernels.hip: sk = NTT(s) bytes || pk || H(pk) || z (kosk.cpp:62-69)
// back to the prover's witness s, e of t = A s + e (kosk.cpp:33-44), and the check that both are in the key generation's range.
// Like kosk_kem_dev.hpp everything here is KOSK_HD and written per work item (`tid` of `nthr` cooperating threads, barriers through
// KEM_SYNC): a host build runs a whole block as tid 0 of 1, which is how tools/witness_host_model.cpp runs these very functions
// without a GPU.
//
// Arithmetic: canonical residues in [0, q), the plain zetas and the plain base multiplication of kosk_kem_dev.hpp.  The reference forms
// t-hat = tomont(A o s-hat) + e-hat (kosk.cpp:41-44): tomont cancels the Montgomery factor of the base multiplication, so on residues
//   e-hat_i = t-hat_i - sum_j A[i][j] o s-hat_j,      s = NTT^-1(s-hat),   e = NTT^-1(e-hat)      (true inverses: the factor 128^-1 included).
//
// Secrets: no branch and no address below depends on s-hat, s, e or the outcome of the range check.  Centring and the range test are
// sign-mask arithmetic, the verdict is an OR over all coefficients (recover_block returns this thread's part; the caller reduces),
// and the zero-fill of a rejected key is a mask (store_block).  A and t are public.
#pragma once
#include "kosk_kem_dev.hpp"

namespace kosk {
namespace wit {

using namespace kem;

// eight u16 to a 16-byte aligned address as ONE 16-byte store, in LDS and in global memory (a vector type: the compiler splits some of
// store16x8's struct stores into four 4-byte stores)
typedef uint32_t Vec4 __attribute__((vector_size(16)));
KOSK_HD inline void store16x8_wide(void *p, const uint32_t (&c)[8])
{
    const Vec4 v = {c[0] | (c[1] << 16), c[2] | (c[3] << 16), c[4] | (c[5] << 16), c[6] | (c[7] << 16)};
    *reinterpret_cast<Vec4 *>(p) = v;
}

// One workgroup, one key.  LDS tile L: 2 K polynomials of 256 u16 -- s-hat[K] | e-hat[K], afterwards s[K] | e[K] as centred int16.
//   sk : the record's first 384 K bytes, s-hat as 12-bit fields (any value: folded mod q), 4-byte aligned
//   A  : A[K][K][256] int16 in [0, q), row-major as the key generation multiplies it (t_i = sum_j A[i][j] o s-hat_j), 16-byte aligned
//   t  : t-hat[K][256] u16 as the 12-bit fields of the pk stand (any value: folded mod q), 16-byte aligned
// Returns non-zero iff one of the coefficients this thread looked at lies outside [-eta1, eta1].
KOSK_HD inline uint32_t recover_block(const Dims &D, uint16_t *L, int tid, int nthr, const uint8_t *sk, const int16_t *A, const uint16_t *t)
{
    const int K = D.K;
    for (int w = tid; w < 2 * K * 32; w += nthr) {
        const int o = w >> 5, g = w & 31; // (o, g) are functions of the thread index only
        uint32_t out[8];
        if (o < K) {
            load12x8(sk + o * 384 + 12 * g, out);
        } else {
            const int i = o - K;
            uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, th[8];
            for (int j = 0; j < K; j++) {
                uint32_t a[8], b[8];
                load16x8(A + ((i * K + j) * 256 + 8 * g), a);
                load12x8(sk + j * 384 + 12 * g, b);
                basemul8_acc(acc, a, b, g);
            }
            load16x8(t + i * 256 + 8 * g, th);
#pragma unroll
            for (int c = 0; c < 8; c++) out[c] = csub(csub(th[c] & 0xFFFu) + (uint32_t)Q - acc[c]);
        }
        store16x8_wide(L + o * 256 + 8 * g, out);
    }
    KEM_SYNC();
    invntt_tile(L, 2 * K, tid, nthr);
    uint32_t bad = 0;
    const int32_t eta = D.eta1;
    for (int w = tid; w < 2 * K * 32; w += nthr) {
        uint32_t x[8];
        load16x8(L + 8 * w, x);
#pragma unroll
        for (int c = 0; c < 8; c++) {
            const int32_t r = (int32_t)mulq(x[c], INV128);
            const int32_t v = r - (((Q / 2 - r) >> 31) & Q);        // centred: [-(q-1)/2, (q-1)/2]
            bad |= (uint32_t)((eta - v) | (eta + v)) >> 31;          // the sign bit of either difference: |v| > eta1
            x[c] = (uint32_t)v & 0xFFFFu;
        }
        store16x8_wide(L + 8 * w, x); // this thread's own eight coefficients: nobody else reads them before the caller's barrier
    }
    return bad;
}

// all ones iff the key's verdict `bad` (the OR of every thread's recover_block) is zero
KOSK_HD inline uint32_t keep_mask(uint32_t bad) { return ((bad | (0u - bad)) >> 31) - 1u; }

// s then e as centred int16 to se (16-byte aligned), all zero for a rejected key; the embedded pk bytes to pk_out (16-byte aligned;
// pk_bytes is a multiple of 16 for every K); ok = 1 / 0.  pk_in = sk + 384 K.
KOSK_HD inline void store_block(const Dims &D, const uint16_t *L, int tid, int nthr, uint32_t bad, const uint8_t *pk_in, int16_t *se, uint8_t *pk_out,
                                uint8_t *ok)
{
    const uint32_t keep = keep_mask(bad);
    for (int w = tid; w < 2 * D.K * 32; w += nthr) {
        uint32_t x[8];
        load16x8(L + 8 * w, x);
#pragma unroll
        for (int c = 0; c < 8; c++) x[c] &= keep;
        store16x8_wide(se + 8 * w, x);
    }
    for (int i = tid; i < D.pk / 16; i += nthr) reinterpret_cast<U128 *>(pk_out)[i] = reinterpret_cast<const U128 *>(pk_in)[i];
    if (tid == 0) *ok = (uint8_t)(keep & 1u);
}

} // namespace wit
} // namespace kosk
