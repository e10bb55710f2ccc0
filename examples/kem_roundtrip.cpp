// The registrar's flow on the C ABI (include/kosk_mi355x.h), end to end on one handle:
//   1. a client makes N key pairs with proofs of knowledge      kosk_verifiable_keygen_batch
//   2. the registrar verifies the proofs (one of them damaged)  kosk_verify_batch
//   3. and encapsulates to the keys it accepted, in HBM         kosk_kem_enc_verified
//   4. the client decapsulates                                  kosk_kem_dec_batch
//   5. both sides hold the same shared secrets
// plus the one-item source-compatible face (kosk_compat.hpp: crypto_kem_enc / crypto_kem_dec).
//   kem_roundtrip [kyber_k = 3] [n = 8]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

static int g_k = 3;
#define KYBER_K 3 /* the compat face is compiled for one parameter set; it is exercised when kyber_k == 3 */
#include "kosk_compat.hpp"

extern "C" void randombytes(uint8_t *out, size_t outlen)
{
    static std::mt19937_64 rng(20260101); // a deterministic stand-in: this is an example, not a key generator
    for (size_t i = 0; i < outlen; i++) out[i] = (uint8_t)rng();
}

#define MUST(x)                                                                       \
    do {                                                                              \
        if (x) {                                                                      \
            fprintf(stderr, "%s: %s\n", #x, kosk_last_error(h));                      \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

int main(int argc, char **argv)
{
    g_k = argc > 1 ? atoi(argv[1]) : 3;
    const int n = argc > 2 ? atoi(argv[2]) : 8;
    if (g_k < 2 || g_k > 4 || n < 2) { fprintf(stderr, "usage: kem_roundtrip [2|3|4] [n >= 2]\n"); return 2; }
    const size_t pkb = kosk_pk_bytes(g_k), skb = kosk_sk_bytes(g_k), pib = kosk_proof_bytes(g_k), ctb = kosk_ct_bytes(g_k);
    kosk_ctx *h = nullptr;
    if (kosk_create(&h, 0, g_k, n)) { fprintf(stderr, "kosk_create: %s\n", kosk_last_error(nullptr)); return 1; }
    kosk_set_randombytes(h, [](void *, uint8_t *out, size_t len) { randombytes(out, len); }, nullptr);
    kosk_set_entropy(h, KOSK_ENTROPY_SEED);
    std::vector<uint8_t> pk(n * pkb), sk(n * skb), pi(n * pib), ok(n), ct(n * ctb), ss(n * KOSK_SS_BYTES), ss2(n * KOSK_SS_BYTES), done(n);
    MUST(kosk_verifiable_keygen_batch(h, n, nullptr, 0, pk.data(), sk.data(), pi.data()));
    pi[1 * pib + 1000] ^= 1; // proof 1 arrives damaged
    MUST(kosk_verify_batch(h, n, pi.data(), pk.data(), ok.data()));
    MUST(kosk_kem_enc_verified(h, n, nullptr, ct.data(), ss.data(), done.data()));
    MUST(kosk_kem_dec_batch(h, n, ct.data(), sk.data(), ss2.data()));
    int accepted = 0, agree = 0, bad = 0;
    for (int b = 0; b < n; b++) {
        if (done[b] != ok[b]) bad++;
        if (!done[b]) {
            for (size_t i = 0; i < ctb; i++) bad += ct[b * ctb + i] != 0;
            continue;
        }
        accepted++;
        agree += memcmp(&ss[b * KOSK_SS_BYTES], &ss2[b * KOSK_SS_BYTES], KOSK_SS_BYTES) == 0;
    }
    printf("[kem] kyber_k %d: %d proofs, %d accepted, %d shared secrets agree\n", g_k, n, accepted, agree);
    if (bad || done[1] || accepted != n - 1 || agree != accepted) { printf("[result] kem roundtrip FAILED\n"); return 1; }
    long enc = 0, dec = 0;
    kosk_path_count(h, 12, &enc);
    kosk_path_count(h, 13, &dec);
    printf("[kem] launch groups: enc %ld dec %ld\n", enc, dec);
    kosk_destroy(h);
    if (g_k == KYBER_K) { // the reference's own names, one item, process-wide handle
        kyber_keypair kp;
        std::vector<uint8_t> proof(MPCITH_PROOF_SIZE);
        kyber_verifiable_keygen(&kp, proof.data());
        uint8_t c[KYBER_CIPHERTEXTBYTES], k1[KYBER_SSBYTES], k2[KYBER_SSBYTES], k3[KYBER_SSBYTES], coins[KYBER_SYMBYTES];
        crypto_kem_enc(c, k1, kp.pk);
        crypto_kem_dec(k2, c, kp.sk);
        bool good = kyber_kosk_verify(proof.data(), kp.pk) && !memcmp(k1, k2, sizeof k1) && sizeof c == kosk_ct_bytes(KYBER_K);
        randombytes(coins, sizeof coins);
        crypto_kem_enc_derand(c, k3, kp.pk, coins);
        crypto_kem_dec(k2, c, kp.sk);
        good = good && !memcmp(k2, k3, sizeof k2) && memcmp(k1, k3, sizeof k1);
        printf("[compat] crypto_kem_enc / crypto_kem_enc_derand / crypto_kem_dec agree = %d\n", (int)good);
        if (!good) { printf("[result] kem roundtrip FAILED\n"); return 1; }
    }
    printf("[result] kem roundtrip success\n");
    return 0;
}
