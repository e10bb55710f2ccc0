// Host build of the key-pair and key-check device functions (csrc/kosk_kem_dev.hpp): the same code k_kem_kg_hash, k_kem_keypair,
// k_kem_hpk and k_kem_check of kosk_kem_kernels.hip run, one "workgroup" executed as thread 0 of 1, in their launch order.
// tests/test_kem_keypair_host.py compiles this into a shared object and checks it against tests/golden/kem_keypair_v1.json, so the
// arithmetic, the packing and the range test are pinned on machines without a GPU.
//
//   c++ -O2 -std=c++20 -shared -fPIC -I mpcith_kyber_kosk_amd/csrc tools/kem_keypair_host_model.cpp -o kem_keypair_host_model.so
#include <cstdint>
#include <cstring>
#include <vector>

#include "kosk_kem_dev.hpp"

using namespace kosk;
using namespace kosk::kem;

// crypto_kem_keypair_derand: coins = d || z.  -2: an entry of A needed more than max_blocks SHAKE128 blocks.
extern "C" int kem_model_keypair(int K, int max_blocks, const uint8_t *coins_in, uint8_t *pk_out, uint8_t *sk_out)
{
    if (K < 2 || K > 4) return -1;
    const Dims D = dims(K);
    alignas(16) static int16_t A[16 * 256], noise[8 * 256];
    alignas(16) static uint16_t L[8 * 256];
    alignas(16) static uint8_t Lb[768 * 4 + 96], pk[384 * 4 + 32], sk[768 * 4 + 96];
    alignas(8) uint8_t coins[64];
    memcpy(coins, coins_in, 64);
    uint64_t d[4], rs[8], rho[4], sigma[4];
    memcpy(d, coins, 32);
    seed_hash_g(d, K, rs);
    for (int l = 0; l < 4; l++) { rho[l] = rs[l]; sigma[l] = rs[4 + l]; }
    for (int t = 0; t < K * K; t++)
        if (!matrix_entry(rho, t % K, t / K, max_blocks, A + t * 256)) return -2;
    for (int t = 0; t < 2 * K; t++) noise_poly(sigma, t, D.eta1, noise + t * 256);
    keypair_block(D, L, Lb, 0, 1, A, noise, reinterpret_cast<const uint8_t *>(rho), coins + 32, pk, sk);
    uint64_t h[4];
    sha3_256_words(pk, D.pk, h);
    memcpy(sk + D.sk - 64, h, 32);
    memcpy(pk_out, pk, (size_t)D.pk);
    memcpy(sk_out, sk, (size_t)D.sk);
    return 0;
}

// kosk_kem_check_pk (is_sk = 0) / kosk_kem_check_sk on one record: the OR over the work items of k_kem_check
extern "C" int kem_model_check(int K, int is_sk, const uint8_t *rec_in)
{
    if (K < 2 || K > 4) return -1;
    const Dims D = dims(K);
    const size_t len = (size_t)(is_sk ? D.sk : D.pk);
    std::vector<uint64_t> buf(len / 8);
    memcpy(buf.data(), rec_in, len);
    const uint8_t *rec = reinterpret_cast<const uint8_t *>(buf.data());
    uint32_t f = 0;
    const int per = K * 32;
    for (int w = 0; w < (is_sk ? 2 : 1) * per; w++) f |= range12x8(rec + 12 * w) * (is_sk && w < per ? 4u : 2u);
    if (is_sk) {
        uint64_t h[4];
        sha3_256_words(rec + D.pvb, D.pk, h);
        const uint8_t *hb = reinterpret_cast<const uint8_t *>(h);
        for (int i = 0; i < 32; i++) f |= nonzero_bit((uint32_t)(hb[i] ^ rec[D.sk - 64 + i]));
    }
    return (int)f;
}
