// The registry tree on the C ABI (include/kosk_mi355x.h, INTEGRATION.md 8.5, format kosk-regtree-v1): a registrar that can show a peer that
// its key is in the set it vouches for, and an auditor one value that pins the whole table.
//   1. n ordinary key pairs, a proof of knowledge for each, one of    kosk_kem_keypair_batch, kosk_prove_keys_batch,
//      them tampered; the registrar checks them                        kosk_verify_batch
//   2. the keys whose proof held are enrolled                          kosk_registry_reserve, kosk_registry_enrol_verified
//   3. the root, and an inclusion path per peer by fingerprint; every  kosk_registry_root, kosk_registry_prove_peers,
//      found path leads to the root, on the host                       kosk_regtree_root_from_path
//   4. one flipped byte in one path: it no longer leads to the root    kosk_regtree_root_from_path
//   5. a peer leaves: the root changes, and the slot's path now        kosk_registry_evict, kosk_registry_prove_slots
//      proves that the slot is empty
//   6. a second handle with the same keys in the same slots gives      kosk_registry_admit, kosk_registry_root
//      the same root
// One line per stage and one for the result, each ending in "= 1" where it holds.
//   registry_audit [kyber_k = 3] [n = 8]
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
    if (k < 2 || k > 4 || n < 3) { fprintf(stderr, "usage: registry_audit [2|3|4] [n >= 3]\n"); return 2; }
    const size_t pkb = kosk_pk_bytes(k), skb = kosk_sk_bytes(k), pib = kosk_proof_bytes(k);
    kosk_ctx *h = nullptr;
    if (kosk_create(&h, 0, k, n)) { fprintf(stderr, "kosk_create: %s\n", kosk_last_error(nullptr)); return 1; }
    kosk_set_entropy(h, KOSK_ENTROPY_SEED);
    const int bad = 1; // the peer whose proof is tampered with
    const int D = kosk_registry_tree_depth(n);
    std::vector<uint8_t> pk(n * pkb), sk(n * skb), pi(n * pib), proven(n), ok(n), status(n), done(n), state(n);
    std::vector<uint8_t> fp(n * 32), paths((size_t)n * D * 32 + 1), root(32), root2(32), got(32);
    std::vector<int32_t> slots(n), found(n);
    int all = 1;
    auto stage = [&](const char *what, bool good) {
        printf("[registry_audit] kyber_k %d, %d peers: %s = %d\n", k, n, what, (int)good);
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
    stage("kosk_registry_enrol_verified: n - 1 keys admitted, the tampered one rejected",
          used == n - 1 && cap == n && status[bad] == KOSK_ENROL_REJECTED && slots[bad] == -1);

    // every peer's fingerprint, the rejected one's included: it must come back as a miss
    for (int b = 0; b < n; b++) kosk_host_sha3_256(&fp[b * 32], &pk[b * pkb], pkb);
    MUST(kosk_registry_root(h, root.data(), &used, &cap));
    MUST(kosk_registry_prove_peers(h, n, fp.data(), found.data(), paths.data(), done.data(), root2.data()));
    bool leads = used == n - 1 && cap == n && !memcmp(root.data(), root2.data(), 32);
    for (int b = 0; b < n; b++) {
        if (b == bad) { leads = leads && done[b] == 0 && found[b] == -1; continue; }
        leads = leads && done[b] == 1 && found[b] == slots[b] &&
                kosk_regtree_root_from_path(k, D, found[b], &fp[b * 32], &paths[(size_t)b * D * 32], got.data()) == 0 && !memcmp(got.data(), root.data(), 32);
    }
    stage("kosk_registry_root + kosk_registry_prove_peers: every enrolled peer's path leads to the root, the rejected peer is a miss", leads);

    const int victim = 0; // an enrolled peer (bad = 1)
    paths[(size_t)victim * D * 32 + 5] ^= 0x40;
    const bool broken = kosk_regtree_root_from_path(k, D, found[victim], &fp[victim * 32], &paths[(size_t)victim * D * 32], got.data()) == 0 &&
                        memcmp(got.data(), root.data(), 32) != 0;
    stage("one flipped byte in a path: it no longer leads to the root", broken);

    const int32_t gone = slots[victim];
    MUST(kosk_registry_evict(h, 1, &gone));
    MUST(kosk_registry_prove_slots(h, 1, &gone, state.data(), nullptr, paths.data(), root2.data()));
    const bool emptied = memcmp(root.data(), root2.data(), 32) != 0 && state[0] == 0 &&
                         kosk_regtree_root_from_path(k, D, gone, nullptr, paths.data(), got.data()) == 0 && !memcmp(got.data(), root2.data(), 32) &&
                         kosk_regtree_root_from_path(k, D, gone, &fp[victim * 32], paths.data(), got.data()) == 0 && memcmp(got.data(), root2.data(), 32) != 0;
    stage("kosk_registry_evict: the root changes, and the slot's path proves that it is empty", emptied);

    // a second registrar that holds the same keys in the same slots
    kosk_ctx *h1 = h;
    kosk_ctx *h2 = nullptr;
    if (kosk_create(&h2, 0, k, n)) { fprintf(stderr, "kosk_create: %s\n", kosk_last_error(nullptr)); return 1; }
    h = h2;
    std::vector<uint8_t> accept(n);
    std::vector<int32_t> where(n);
    for (int b = 0; b < n; b++) { accept[b] = b != bad && b != victim; where[b] = accept[b] ? slots[b] : n - 1 - b; }
    // the positions that are not accepted need distinct slot ids all the same: give them ids no accepted key has
    {
        std::vector<uint8_t> taken(n, 0);
        for (int b = 0; b < n; b++) if (accept[b]) taken[where[b]] = 1;
        int next = 0;
        for (int b = 0; b < n; b++) {
            if (accept[b]) continue;
            while (taken[next]) next++;
            where[b] = next; taken[next] = 1;
        }
    }
    MUST(kosk_registry_reserve(h, n));
    MUST(kosk_registry_admit(h, n, pk.data(), accept.data(), where.data()));
    MUST(kosk_registry_root(h, got.data(), &used, &cap));
    stage("a second handle with the same keys in the same slots: the same root", used == n - 2 && cap == n && !memcmp(got.data(), root2.data(), 32));
    kosk_destroy(h2);
    kosk_destroy(h1);
    printf("[result] registry_audit success = %d\n", all);
    return all ? 0 : 1;
}
