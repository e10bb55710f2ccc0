// The verified-key registry on the C ABI (include/kosk_mi355x.h): a registrar enrols n peers once and talks to
// them again and again.
//   1. n ordinary key pairs                                         kosk_kem_keypair_batch
//   2. a proof of knowledge for each, one of them tampered           kosk_prove_keys_batch
//   3. the registrar checks them                                    kosk_verify_batch
//   4. the keys whose proof held enter the registry, peer b in      kosk_registry_reserve, kosk_registry_admit_verified,
//      slot n - 1 - b; the pk bytes, H(pk) and A^T are decoded once  kosk_registry_level
//   5. two rounds of encapsulations by slot under different coins    kosk_kem_enc_slots
//   6. every enrolled peer decapsulates both to the same secrets     kosk_kem_dec_batch
//   7. the rejected peer's slot is empty: done = 0, zero outputs     kosk_registry_read
//   8. a peer leaves                                                kosk_registry_evict
// One line per stage and one for the result, each ending in "= 1" where it holds.
//   registry_enrol [kyber_k = 3] [n = 8]
#include <cstdio>
#include <cstdlib>
#include <cstring>
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
    if (k < 2 || k > 4 || n < 3) { fprintf(stderr, "usage: registry_enrol [2|3|4] [n >= 3]\n"); return 2; }
    const size_t pkb = kosk_pk_bytes(k), skb = kosk_sk_bytes(k), pib = kosk_proof_bytes(k), ctb = kosk_ct_bytes(k);
    kosk_ctx *h = nullptr;
    if (kosk_create(&h, 0, k, n)) { fprintf(stderr, "kosk_create: %s\n", kosk_last_error(nullptr)); return 1; }
    kosk_set_entropy(h, KOSK_ENTROPY_SEED);
    const int bad = 1; // the peer whose proof is tampered with
    std::vector<uint8_t> pk(n * pkb), sk(n * skb), pi(n * pib), proven(n), ok(n), admitted(n), done(n), state(n);
    std::vector<uint8_t> ct(n * ctb), ss(n * KOSK_SS_BYTES), ct2(n * ctb), ss2(n * KOSK_SS_BYTES), dec(n * KOSK_SS_BYTES), dec2(n * KOSK_SS_BYTES);
    std::vector<int32_t> slots(n);
    for (int b = 0; b < n; b++) slots[b] = n - 1 - b;
    int all = 1;
    auto stage = [&](const char *what, bool good) {
        printf("[registry_enrol] kyber_k %d, %d peers: %s = %d\n", k, n, what, (int)good);
        all &= (int)good;
    };

    MUST(kosk_kem_keypair_batch(h, n, nullptr, pk.data(), sk.data()));
    MUST(kosk_prove_keys_batch(h, n, sk.data(), nullptr, 0, pi.data(), proven.data()));
    pi[bad * pib + 1000] ^= 1; // proof 1 arrives damaged
    MUST(kosk_verify_batch(h, n, pi.data(), pk.data(), ok.data()));
    int good = 0;
    for (int b = 0; b < n; b++) good += proven[b] == 1 && ok[b] == (b != bad);
    stage("kosk_prove_keys_batch + kosk_verify_batch: every proof verifies but the tampered one", good == n);

    int used = -1, cap = -1;
    MUST(kosk_registry_reserve(h, n));
    MUST(kosk_registry_admit_verified(h, n, slots.data(), admitted.data()));
    MUST(kosk_registry_level(h, &used, &cap));
    long admits = 0;
    kosk_path_count(h, 27, &admits);
    stage("kosk_registry_admit_verified: n - 1 keys admitted with one launch of k_registry_admit", admitted == ok && used == n - 1 && cap == n && admits == 1);

    MUST(kosk_kem_enc_slots(h, n, slots.data(), nullptr, ct.data(), ss.data(), done.data()));
    MUST(kosk_kem_enc_slots(h, n, slots.data(), nullptr, ct2.data(), ss2.data(), done.data()));
    MUST(kosk_kem_dec_batch(h, n, ct.data(), sk.data(), dec.data()));
    MUST(kosk_kem_dec_batch(h, n, ct2.data(), sk.data(), dec2.data()));
    int agree = 0;
    for (int b = 0; b < n; b++)
        agree += b == bad || (done[b] == 1 && !memcmp(&ss[b * KOSK_SS_BYTES], &dec[b * KOSK_SS_BYTES], KOSK_SS_BYTES) &&
                              !memcmp(&ss2[b * KOSK_SS_BYTES], &dec2[b * KOSK_SS_BYTES], KOSK_SS_BYTES) &&
                              memcmp(&ss[b * KOSK_SS_BYTES], &ss2[b * KOSK_SS_BYTES], KOSK_SS_BYTES));
    stage("two rounds of kosk_kem_enc_slots + kosk_kem_dec_batch: equal secrets, fresh every round", agree == n);

    const std::vector<uint8_t> zct(ctb, 0), zss(KOSK_SS_BYTES, 0), zpk(pkb, 0);
    std::vector<uint8_t> rpk(n * pkb), rh(n * 32);
    MUST(kosk_registry_read(h, n, slots.data(), state.data(), rpk.data(), rh.data()));
    bool kept = true;
    for (int b = 0; b < n; b++) kept = kept && state[b] == (b != bad) && !memcmp(&rpk[b * pkb], b == bad ? zpk.data() : &pk[b * pkb], pkb);
    stage("the rejected peer: done = 0, zero ct and ss, an empty slot; the others hold their pk bytes",
          done[bad] == 0 && !memcmp(&ct[bad * ctb], zct.data(), ctb) && !memcmp(&ss[bad * KOSK_SS_BYTES], zss.data(), KOSK_SS_BYTES) && kept);

    MUST(kosk_registry_evict(h, 1, &slots[0]));
    MUST(kosk_registry_level(h, &used, &cap));
    MUST(kosk_kem_enc_slots(h, n, slots.data(), nullptr, ct.data(), ss.data(), done.data()));
    long groups = 0;
    kosk_path_count(h, 28, &groups);
    stage("kosk_registry_evict: peer 0 is gone, the others are served as before", used == n - 2 && done[0] == 0 && done[n - 1] == 1 && groups == 3);
    kosk_destroy(h);
    printf("[result] registry_enrol success = %d\n", all);
    return all ? 0 : 1;
}
