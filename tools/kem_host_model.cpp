// Host build of the KEM device functions (csrc/kosk_kem_dev.hpp): the same code the gfx950 kernels run, one "workgroup" executed as
// thread 0 of 1, in the launch order of kosk_kem_kernels.hip.  tests/test_kem_host.py compiles this into a shared object and checks
// it against tests/golden/kem_vectors_v1.json, so the arithmetic and the sponges are pinned on machines without a GPU.
//
//   c++ -O2 -std=c++20 -shared -fPIC -I mpcith_kyber_kosk_amd/csrc tools/kem_host_model.cpp -o kem_host_model.so
#include <cstdint>
#include <cstring>
#include <vector>

#include "kosk_kem_dev.hpp"

using namespace kosk;
using namespace kosk::kem;

namespace {

struct Scratch {
    alignas(16) int16_t A[16 * 256];
    alignas(16) int16_t noise[9 * 256];
    alignas(16) uint16_t L[10 * 256];
    alignas(16) uint8_t Lb[288];
};

// gen_matrix (transposed) + the 2 K + 1 noise polynomials of indcpa_enc
bool sample(const Dims &D, const uint8_t *pk, const uint64_t (&coins)[4], Scratch &w)
{
    uint64_t rho[4];
    memcpy(rho, pk + D.pvb, 32);
    for (int i = 0; i < D.K; i++)
        for (int j = 0; j < D.K; j++)
            if (!matrix_entry(rho, i, j, 32, w.A + (i * D.K + j) * 256)) return false;
    for (int t = 0; t < 2 * D.K + 1; t++) noise_poly(coins, t, t < D.K ? D.eta1 : 2, w.noise + t * 256);
    return true;
}

} // namespace

extern "C" int kem_model_enc(int K, const uint8_t *pk_in, const uint8_t *m_in, uint8_t *ct, uint8_t *ss)
{
    if (K < 2 || K > 4) return -1;
    const Dims D = dims(K);
    std::vector<uint64_t> pkw((size_t)D.pk / 8);
    memcpy(pkw.data(), pk_in, (size_t)D.pk);
    const uint8_t *pk = reinterpret_cast<const uint8_t *>(pkw.data());
    uint64_t m[4], h[4], kr[8], coins[4];
    memcpy(m, m_in, 32);
    sha3_256_words(pk, D.pk, h);
    hash_g64(m, h, kr);
    for (int l = 0; l < 4; l++) coins[l] = kr[4 + l];
    Scratch w;
    if (!sample(D, pk, coins, w)) return -2;
    encrypt_block(D, w.L, 0, 1, pk, w.A, w.noise, m_in, ct, nullptr);
    memcpy(ss, kr, 32);
    return 0;
}

extern "C" int kem_model_dec(int K, const uint8_t *ct_in, const uint8_t *sk_in, uint8_t *ss)
{
    if (K < 2 || K > 4) return -1;
    const Dims D = dims(K);
    std::vector<uint64_t> skw((size_t)D.sk / 8), ctw((size_t)D.ct / 8);
    memcpy(skw.data(), sk_in, (size_t)D.sk);
    memcpy(ctw.data(), ct_in, (size_t)D.ct);
    const uint8_t *sk = reinterpret_cast<const uint8_t *>(skw.data()), *ct = reinterpret_cast<const uint8_t *>(ctw.data());
    const uint8_t *pk = sk + D.pvb;
    Scratch w;
    decrypt_block(D, w.L, w.Lb, 0, 1, ct, sk);
    uint64_t m[4], h[4], kr[8], coins[4], rk[4];
    memcpy(m, w.Lb + 256, 32);
    memcpy(h, sk + D.sk - 64, 32);
    hash_g64(m, h, kr);
    for (int l = 0; l < 4; l++) coins[l] = kr[4 + l];
    if (!sample(D, pk, coins, w)) return -2;
    const uint32_t diff = encrypt_block(D, w.L, 0, 1, pk, w.A, w.noise, w.Lb + 256, nullptr, ct);
    rkprf(sk + D.sk - 32, ct, D.ct, rk);
    const uint8_t *kb = reinterpret_cast<const uint8_t *>(kr), *rb = reinterpret_cast<const uint8_t *>(rk);
    for (int i = 0; i < 32; i++) ss[i] = select_ss(diff, kb[i], rb[i]);
    return 0;
}

// indcpa_dec alone (kyber/indcpa.c:317-336): m' of any ciphertext under the s-hat of sk.  A decapsulation that rejects returns
// SHAKE256(z || ct) whatever m' was, so this is where decompress (every code), the s-hat fold and tomsg show on foreign ciphertexts.
extern "C" int kem_model_indcpa_dec(int K, const uint8_t *ct_in, const uint8_t *sk_in, uint8_t *m)
{
    if (K < 2 || K > 4) return -1;
    const Dims D = dims(K);
    std::vector<uint64_t> skw((size_t)D.sk / 8), ctw((size_t)D.ct / 8);
    memcpy(skw.data(), sk_in, (size_t)D.sk);
    memcpy(ctw.data(), ct_in, (size_t)D.ct);
    Scratch w;
    decrypt_block(D, w.L, w.Lb, 0, 1, reinterpret_cast<const uint8_t *>(ctw.data()), reinterpret_cast<const uint8_t *>(skw.data()));
    memcpy(m, w.Lb + 256, 32);
    return 0;
}

// the compression expression over its whole domain, for the test that pins it: out[d_index][x], d in {4, 5, 10, 11}
extern "C" void kem_model_compress_table(uint16_t *out)
{
    const int ds[4] = {4, 5, 10, 11};
    for (int k = 0; k < 4; k++)
        for (int x = 0; x < Q; x++) out[k * Q + x] = (uint16_t)compress((uint32_t)x, ds[k]);
}
