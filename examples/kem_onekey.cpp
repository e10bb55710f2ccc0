// KEM with one resident key on the C ABI (include/kosk_mi355x.h): a party that owns one ML-KEM key and answers
// many peers with it.
//   1. one key pair                                                 kosk_kem_keypair_batch
//   2. the sk goes into the handle's key slot, once                 kosk_kem_key_set, kosk_kem_key_state
//   3. n encapsulations to it                                       kosk_kem_enc_key
//   4. n decapsulations with it                                     kosk_kem_dec_key (equal secrets)
//   5. the same bytes as the per-item calls on n copies of the key  kosk_kem_enc_batch, kosk_kem_dec_batch
//   6. the audit finds z; after the wipe it does not, the slot      kosk_secret_scan, kosk_wipe_secrets
//      serves as a public key and decapsulation refuses
// One line per stage and one for the result, each ending in "= 1" where it holds.
//   kem_onekey [kyber_k = 3] [n = 8]
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
    const int n = argc > 2 ? atoi(argv[2]) : 8;
    if (k < 2 || k > 4 || n < 1) { fprintf(stderr, "usage: kem_onekey [2|3|4] [n >= 1]\n"); return 2; }
    const size_t pkb = kosk_pk_bytes(k), skb = kosk_sk_bytes(k), ctb = kosk_ct_bytes(k);
    kosk_ctx *h = nullptr;
    if (kosk_create(&h, 0, k, 1)) { fprintf(stderr, "kosk_create: %s\n", kosk_last_error(nullptr)); return 1; }
    std::mt19937_64 rng(20261019); // a deterministic stand-in: this is an example, not a key generator
    std::vector<uint8_t> kg(64), coins((size_t)n * 32);
    for (auto *v : {&kg, &coins})
        for (auto &x : *v) x = (uint8_t)rng();
    std::vector<uint8_t> pk(pkb), sk(skb), ct(n * ctb), ss(n * 32), ss2(n * 32), ct3(n * ctb), ss3(n * 32), ss4(n * 32);
    int all = 1;
    auto stage = [&](const char *what, bool good) {
        printf("[kem_onekey] kyber_k %d, %d items: %s = %d\n", k, n, what, (int)good);
        all &= (int)good;
    };

    MUST(kosk_kem_keypair_batch(h, 1, kg.data(), pk.data(), sk.data()));
    stage("kosk_kem_keypair_batch: the slot is empty", kosk_kem_key_state(h) == KOSK_KEM_KEY_NONE);
    MUST(kosk_kem_key_set(h, nullptr, sk.data()));
    long setups = 0;
    kosk_path_count(h, 19, &setups);
    stage("kosk_kem_key_set: the sk is resident, one launch of k_kem_key_setup", kosk_kem_key_state(h) == KOSK_KEM_KEY_SK && setups == 1);
    MUST(kosk_kem_enc_key(h, n, coins.data(), ct.data(), ss.data()));
    MUST(kosk_kem_dec_key(h, n, ct.data(), ss2.data()));
    stage("kosk_kem_enc_key + kosk_kem_dec_key: equal secrets", ss == ss2);

    std::vector<uint8_t> pks(n * pkb), sks(n * skb);
    for (int b = 0; b < n; b++) { memcpy(&pks[b * pkb], pk.data(), pkb); memcpy(&sks[b * skb], sk.data(), skb); }
    MUST(kosk_kem_enc_batch(h, n, pks.data(), coins.data(), ct3.data(), ss3.data()));
    MUST(kosk_kem_dec_batch(h, n, ct.data(), sks.data(), ss4.data()));
    stage("the per-item calls on n copies of the key return the same bytes", ct3 == ct && ss3 == ss && ss4 == ss2);

    const uint8_t *z = &sk[skb - 32];
    long before = 0, after = 0;
    MUST(kosk_secret_scan(h, z, 32, &before));
    MUST(kosk_wipe_secrets(h));
    MUST(kosk_secret_scan(h, z, 32, &after));
    stage("kosk_secret_scan: z is found before kosk_wipe_secrets and not after", before >= 1 && after == 0);
    MUST(kosk_kem_enc_key(h, n, coins.data(), ct3.data(), ss3.data()));
    const int refused = kosk_kem_dec_key(h, n, ct.data(), ss4.data());
    stage("after the wipe: state PK, the same encapsulations, decapsulation refuses (key was wiped)",
          kosk_kem_key_state(h) == KOSK_KEM_KEY_PK && ct3 == ct && ss3 == ss && refused == -1 && strstr(kosk_last_error(h), "wiped") != nullptr);
    MUST(kosk_kem_key_clear(h));
    stage("kosk_kem_key_clear: the slot is empty", kosk_kem_key_state(h) == KOSK_KEM_KEY_NONE);
    kosk_destroy(h);
    printf("[result] kem_onekey success = %d\n", all);
    return all ? 0 : 1;
}
