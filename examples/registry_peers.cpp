// The registry by fingerprint on the C ABI (include/kosk_mi355x.h): a registrar that knows its peers by SHA3-256(pk)
// and never invents a slot number.
//   1. n ordinary key pairs, a proof of knowledge for each, one of    kosk_kem_keypair_batch, kosk_prove_keys_batch,
//      them tampered; the registrar checks them                        kosk_verify_batch
//   2. the keys whose proof held are enrolled; the library picks the   kosk_registry_reserve, kosk_registry_enrol_verified
//      slots, lowest first
//   3. the same batch once more: every key is a duplicate, in the      kosk_verify_batch, kosk_registry_enrol_verified
//      slot it has
//   4. encapsulations by fingerprint; every enrolled peer              kosk_registry_read, kosk_kem_enc_peers, kosk_kem_dec_batch
//      decapsulates to the same secret
//   5. a fingerprint nobody enrolled: done = 0, zero outputs           kosk_kem_enc_peers
//   6. a peer leaves: its fingerprint is not found any more            kosk_registry_evict, kosk_registry_find
// One line per stage and one for the result, each ending in "= 1" where it holds.
//   registry_peers [kyber_k = 3] [n = 8]
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
    if (k < 2 || k > 4 || n < 3) { fprintf(stderr, "usage: registry_peers [2|3|4] [n >= 3]\n"); return 2; }
    const size_t pkb = kosk_pk_bytes(k), skb = kosk_sk_bytes(k), pib = kosk_proof_bytes(k), ctb = kosk_ct_bytes(k);
    kosk_ctx *h = nullptr;
    if (kosk_create(&h, 0, k, n)) { fprintf(stderr, "kosk_create: %s\n", kosk_last_error(nullptr)); return 1; }
    kosk_set_entropy(h, KOSK_ENTROPY_SEED);
    const int bad = 1; // the peer whose proof is tampered with
    std::vector<uint8_t> pk(n * pkb), sk(n * skb), pi(n * pib), proven(n), ok(n), status(n), status2(n), done(n + 1), state(n);
    std::vector<uint8_t> ct((n + 1) * ctb), ss((n + 1) * KOSK_SS_BYTES), dec(n * KOSK_SS_BYTES), fp((n + 1) * 32);
    std::vector<int32_t> slots(n), slots2(n), found(n + 1);
    int all = 1;
    auto stage = [&](const char *what, bool good) {
        printf("[registry_peers] kyber_k %d, %d peers: %s = %d\n", k, n, what, (int)good);
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
    MUST(kosk_registry_enrol_verified(h, n, slots.data(), status.data()));
    MUST(kosk_registry_level(h, &used, &cap));
    bool picked = used == n - 1 && cap == n;
    for (int b = 0, next = 0; b < n; b++) {
        if (b == bad) picked = picked && status[b] == KOSK_ENROL_REJECTED && slots[b] == -1;
        else picked = picked && status[b] == KOSK_ENROL_ADMITTED && slots[b] == next++;
    }
    stage("kosk_registry_enrol_verified: n - 1 keys admitted into slots 0 .. n - 2, the tampered one rejected", picked);

    MUST(kosk_verify_batch(h, n, pi.data(), pk.data(), ok.data()));
    MUST(kosk_registry_enrol_verified(h, n, slots2.data(), status2.data()));
    MUST(kosk_registry_level(h, &used, &cap));
    bool dup = used == n - 1;
    for (int b = 0; b < n; b++) dup = dup && slots2[b] == slots[b] && status2[b] == (b == bad ? KOSK_ENROL_REJECTED : KOSK_ENROL_DUPLICATE);
    stage("the same batch again: every key is a duplicate in the slot it has, nothing is written", dup);

    // the peers' fingerprints as the registry stores them: SHA3-256 of the pk bytes; the rejected peer's slot is -1, so read the others
    std::vector<int32_t> live;
    std::vector<int> who;
    for (int b = 0; b < n; b++)
        if (b != bad) { live.push_back(slots[b]); who.push_back(b); }
    const int m = (int)live.size();
    MUST(kosk_registry_read(h, m, live.data(), state.data(), nullptr, fp.data()));
    MUST(kosk_kem_enc_peers(h, m, fp.data(), nullptr, ct.data(), ss.data(), done.data()));
    std::vector<uint8_t> sk_live(m * skb);
    for (int i = 0; i < m; i++) memcpy(&sk_live[i * skb], &sk[who[i] * skb], skb);
    MUST(kosk_kem_dec_batch(h, m, ct.data(), sk_live.data(), dec.data()));
    int agree = 0;
    for (int i = 0; i < m; i++) agree += done[i] == 1 && !memcmp(&ss[i * KOSK_SS_BYTES], &dec[i * KOSK_SS_BYTES], KOSK_SS_BYTES);
    stage("kosk_kem_enc_peers by fingerprint + kosk_kem_dec_batch: equal secrets", agree == m);

    const std::vector<uint8_t> zct(ctb, 0), zss(KOSK_SS_BYTES, 0);
    for (int i = 0; i < 32; i++) fp[m * 32 + i] = (uint8_t)(fp[i] ^ 0x5a); // nobody's fingerprint, behind the real ones
    MUST(kosk_kem_enc_peers(h, m + 1, fp.data(), nullptr, ct.data(), ss.data(), done.data()));
    stage("an unknown fingerprint: done = 0, zero ct and ss; the others are served",
          done[m] == 0 && done[0] == 1 && !memcmp(&ct[m * ctb], zct.data(), ctb) && !memcmp(&ss[m * KOSK_SS_BYTES], zss.data(), KOSK_SS_BYTES));

    MUST(kosk_registry_find(h, m, fp.data(), found.data()));
    bool before = true;
    for (int i = 0; i < m; i++) before = before && found[i] == live[i];
    MUST(kosk_registry_evict(h, 1, &live[0]));
    MUST(kosk_registry_find(h, m, fp.data(), found.data()));
    long rebuilds = 0;
    kosk_path_count(h, 29, &rebuilds);
    bool after = found[0] == -1;
    for (int i = 1; i < m; i++) after = after && found[i] == live[i];
    stage("kosk_registry_evict: the peer's fingerprint is not found any more, the others are", before && after && rebuilds == 3);
    kosk_destroy(h);
    printf("[result] registry_peers success = %d\n", all);
    return all ? 0 : 1;
}
