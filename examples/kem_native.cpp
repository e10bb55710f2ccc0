// A provisioning line on the C ABI (include/kosk_mi355x.h) that makes ordinary Kyber key pairs first and proves them later, on one handle:
//   1. N key pairs, each with an independent z                    kosk_kem_keypair_batch
//   2. the FIPS 203 input checks on what it made                  kosk_kem_check_sk (all flags zero)
//   3. proofs of knowledge for those keys, then their verification  kosk_prove_keys_batch, kosk_verify_batch
//   4. encapsulation to the verified keys in HBM, decapsulation   kosk_kem_enc_verified, kosk_kem_dec_batch (equal secrets)
// plus, for kyber_k == 3, the one-item source-compatible face (kosk_compat.hpp: crypto_kem_keypair, crypto_kem_enc, crypto_kem_dec).
// One line per stage, ending in "= 1" where it holds.
//   kem_native [kyber_k = 3] [n = 8]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#define KYBER_K 3 /* the compat face is compiled for one parameter set; it is exercised when kyber_k == 3 */
#include "kosk_compat.hpp"

extern "C" void randombytes(uint8_t *out, size_t outlen)
{
    static std::mt19937_64 rng(20260202); // a deterministic stand-in: this is an example, not a key generator
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
    const int k = argc > 1 ? atoi(argv[1]) : 3;
    const int n = argc > 2 ? atoi(argv[2]) : 8;
    if (k < 2 || k > 4 || n < 1) { fprintf(stderr, "usage: kem_native [2|3|4] [n >= 1]\n"); return 2; }
    const size_t pkb = kosk_pk_bytes(k), skb = kosk_sk_bytes(k), pib = kosk_proof_bytes(k), ctb = kosk_ct_bytes(k);
    kosk_ctx *h = nullptr;
    if (kosk_create(&h, 0, k, n)) { fprintf(stderr, "kosk_create: %s\n", kosk_last_error(nullptr)); return 1; }
    kosk_set_randombytes(h, [](void *, uint8_t *out, size_t len) { randombytes(out, len); }, nullptr);
    kosk_set_entropy(h, KOSK_ENTROPY_SEED);
    std::vector<uint8_t> pk(n * pkb), sk(n * skb), flags(n, 0xFF), pi(n * pib), proven(n), ok(n), done(n);
    std::vector<uint8_t> ct(n * ctb), ss(n * KOSK_SS_BYTES), ss2(n * KOSK_SS_BYTES);
    int all = 1;
    auto stage = [&](const char *what, bool good) {
        printf("[kem_native] kyber_k %d, %d items: %s = %d\n", k, n, what, (int)good);
        all &= (int)good;
    };

    MUST(kosk_kem_keypair_batch(h, n, nullptr, pk.data(), sk.data()));
    bool embedded = true;
    for (int b = 0; b < n; b++) embedded = embedded && !memcmp(&sk[b * skb + 384 * k], &pk[b * pkb], pkb);
    stage("kosk_kem_keypair_batch: every sk embeds its pk", embedded);

    MUST(kosk_kem_check_sk(h, n, sk.data(), flags.data()));
    int flagged = 0;
    for (int b = 0; b < n; b++) flagged += flags[b] != 0;
    stage("kosk_kem_check_sk: all flags zero", flagged == 0);

    MUST(kosk_prove_keys_batch(h, n, sk.data(), nullptr, 0, pi.data(), proven.data()));
    MUST(kosk_verify_batch(h, n, pi.data(), pk.data(), ok.data()));
    int good = 0;
    for (int b = 0; b < n; b++) good += proven[b] == 1 && ok[b] == 1;
    stage("kosk_prove_keys_batch + kosk_verify_batch: every key proven and verified", good == n);

    MUST(kosk_kem_enc_verified(h, n, nullptr, ct.data(), ss.data(), done.data()));
    MUST(kosk_kem_dec_batch(h, n, ct.data(), sk.data(), ss2.data()));
    int agree = 0;
    for (int b = 0; b < n; b++) agree += done[b] == 1 && !memcmp(&ss[b * KOSK_SS_BYTES], &ss2[b * KOSK_SS_BYTES], KOSK_SS_BYTES);
    stage("kosk_kem_enc_verified + kosk_kem_dec_batch: equal secrets", agree == n);

    long groups = 0, checks = 0;
    kosk_path_count(h, 15, &groups);
    kosk_path_count(h, 16, &checks);
    stage("launch groups counted (ids 15, 16)", groups >= 1 && checks >= 1);
    kosk_destroy(h);

    if (k == KYBER_K) { // the reference's own names (kyber/kem.h), one item, process-wide handle
        uint8_t cpk[KYBER_PUBLICKEYBYTES], csk[KYBER_SECRETKEYBYTES], c[KYBER_CIPHERTEXTBYTES], k1[KYBER_SSBYTES], k2[KYBER_SSBYTES];
        uint8_t coins[2 * KYBER_SYMBYTES], dpk[KYBER_PUBLICKEYBYTES], dsk[KYBER_SECRETKEYBYTES], dpk2[KYBER_PUBLICKEYBYTES], dsk2[KYBER_SECRETKEYBYTES];
        crypto_kem_keypair(cpk, csk);
        crypto_kem_enc(c, k1, cpk);
        crypto_kem_dec(k2, c, csk);
        bool face = !memcmp(k1, k2, sizeof k1);
        randombytes(coins, sizeof coins);
        crypto_kem_keypair_derand(dpk, dsk, coins);
        crypto_kem_keypair_derand(dpk2, dsk2, coins);
        face = face && !memcmp(dpk, dpk2, sizeof dpk) && !memcmp(dsk, dsk2, sizeof dsk) && !memcmp(dsk + sizeof dsk - 32, coins + 32, 32) &&
               memcmp(dpk, cpk, sizeof dpk);
        stage("compat crypto_kem_keypair / crypto_kem_enc / crypto_kem_dec agree", face);
    }
    printf("[result] kem native %s\n", all ? "success" : "FAILED");
    return all ? 0 : 1;
}
