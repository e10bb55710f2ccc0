// Erasing secrets on the C ABI (include/kosk_mi355x.h), with the audit that shows it happened, on one handle:
//   1. N verifiable key generations from tapes                      kosk_verifiable_keygen_batch
//   2. proofs for those keys again, from fresh tapes                kosk_prove_keys_batch
//   3. a KEM round trip on them                                     kosk_kem_enc_batch, kosk_kem_dec_batch (equal secrets)
//   4. the audit finds a key's z and a tape's first PRF seed        kosk_secret_scan (hits >= 1)
//   5. the wipe; the audit finds neither, and still finds a pk      kosk_wipe_secrets, kosk_secret_scan (0, 0, >= 1)
//   6. the same calls with the wipe at the end of every call        kosk_set_wipe(KOSK_WIPE_CALL): equal proofs, nothing left behind
// One line per stage and one for the result, each ending in "= 1" where it holds.
//   wipe_audit [kyber_k = 3] [n = 3]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "kosk_mi355x.h"

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
    const int n = argc > 2 ? atoi(argv[2]) : 3;
    if (k < 2 || k > 4 || n < 1) { fprintf(stderr, "usage: wipe_audit [2|3|4] [n >= 1]\n"); return 2; }
    const size_t pkb = kosk_pk_bytes(k), skb = kosk_sk_bytes(k), pib = kosk_proof_bytes(k), ctb = kosk_ct_bytes(k), tb = kosk_tape_bytes(k);
    kosk_ctx *h = nullptr;
    if (kosk_create(&h, 0, k, n)) { fprintf(stderr, "kosk_create: %s\n", kosk_last_error(nullptr)); return 1; }
    std::mt19937_64 rng(20261019); // a deterministic stand-in: this is an example, not a key generator
    std::vector<uint8_t> tapes(n * tb), tapes2(n * tb), coins(n * 32);
    for (auto *v : {&tapes, &tapes2, &coins})
        for (auto &x : *v) x = (uint8_t)rng();
    std::vector<uint8_t> pk(n * pkb), sk(n * skb), pi(n * pib), pi2(n * pib), pi3(n * pib), proven(n), ct(n * ctb), ss(n * 32), ss2(n * 32);
    int all = 1;
    auto stage = [&](const char *what, bool good) {
        printf("[wipe_audit] kyber_k %d, %d items: %s = %d\n", k, n, what, (int)good);
        all &= (int)good;
    };
    const uint8_t *z = &sk[(n - 1) * skb + skb - 32], *prf = &tapes2[(n - 1) * tb + 64], *pub = &pk[0];
    long hz = 0, ht = 0, hp = 0;

    MUST(kosk_verifiable_keygen_batch(h, n, tapes.data(), tb, pk.data(), sk.data(), pi.data()));
    MUST(kosk_prove_keys_batch(h, n, sk.data(), tapes2.data(), tb, pi2.data(), proven.data()));
    int good = 0;
    for (int b = 0; b < n; b++) good += proven[b] == 1;
    stage("kosk_verifiable_keygen_batch + kosk_prove_keys_batch: every key proven", good == n);
    MUST(kosk_kem_enc_batch(h, n, pk.data(), coins.data(), ct.data(), ss.data()));
    MUST(kosk_kem_dec_batch(h, n, ct.data(), sk.data(), ss2.data()));
    stage("kosk_kem_enc_batch + kosk_kem_dec_batch: equal secrets", !memcmp(ss.data(), ss2.data(), ss.size()));

    MUST(kosk_secret_scan(h, z, 32, &hz));
    MUST(kosk_secret_scan(h, prf, 32, &ht));
    MUST(kosk_secret_scan(h, pub, 32, &hp));
    stage("kosk_secret_scan before the wipe: z, a tape's PRF seed and a pk are found", hz >= 1 && ht >= 1 && hp >= 1);

    MUST(kosk_wipe_secrets(h));
    MUST(kosk_secret_scan(h, z, 32, &hz));
    MUST(kosk_secret_scan(h, prf, 32, &ht));
    MUST(kosk_secret_scan(h, pub, 32, &hp));
    stage("kosk_wipe_secrets: z and the PRF seed are gone, the pk is still there", hz == 0 && ht == 0 && hp >= 1);

    MUST(kosk_set_wipe(h, KOSK_WIPE_CALL));
    MUST(kosk_prove_keys_batch(h, n, sk.data(), tapes2.data(), tb, pi3.data(), proven.data()));
    MUST(kosk_kem_dec_batch(h, n, ct.data(), sk.data(), ss2.data()));
    MUST(kosk_secret_scan(h, z, 32, &hz));
    MUST(kosk_secret_scan(h, prf, 32, &ht));
    stage("KOSK_WIPE_CALL: the same proofs and secrets, nothing left behind", pi3 == pi2 && !memcmp(ss.data(), ss2.data(), ss.size()) && hz == 0 && ht == 0);

    long wipes = 0;
    kosk_path_count(h, 18, &wipes);
    stage("launches of k_wipe counted (id 18)", wipes >= 3);
    kosk_destroy(h); // always wipes before it frees
    printf("[result] wipe_audit success = %d\n", all);
    return all ? 0 : 1;
}
