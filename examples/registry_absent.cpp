// The sorted tree on the C ABI (include/kosk_mi355x.h, INTEGRATION.md 8.6, format kosk-regsort-v1): a registrar that can show an outsider
// that a key is NOT enrolled -- the second half of the rogue-key defence: "and this key was not enrolled before".
//   1. n ordinary key pairs, a proof of knowledge for each; the        kosk_kem_keypair_batch, kosk_prove_keys_batch,
//      registrar checks them and enrols the keys                       kosk_verify_batch, kosk_registry_enrol_verified
//   2. the sorted root, and a proof of absence for a fingerprint       kosk_registry_sorted_root, kosk_registry_prove_absent,
//      nobody enrolled; it checks on the host                          kosk_regsort_check_proof
//   3. an enrolled fingerprint comes back PRESENT, and the slot the    kosk_registry_prove_absent, kosk_registry_prove_slots,
//      record names leads to the slot tree's root with the same key    kosk_regtree_root_from_path
//   4. one flipped byte in the proof of absence: it proves nothing     kosk_regsort_check_proof
//   5. a peer leaves: under the new root its key is absent, and the    kosk_registry_evict, kosk_registry_prove_absent
//      old record no longer checks
// One line per stage and one for the result, each ending in "= 1" where it holds.
//   registry_absent [kyber_k = 3] [n = 8]
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
    if (k < 2 || k > 4 || n < 3) { fprintf(stderr, "usage: registry_absent [2|3|4] [n >= 3]\n"); return 2; }
    const size_t pkb = kosk_pk_bytes(k), skb = kosk_sk_bytes(k), pib = kosk_proof_bytes(k);
    kosk_ctx *h = nullptr;
    if (kosk_create(&h, 0, k, n)) { fprintf(stderr, "kosk_create: %s\n", kosk_last_error(nullptr)); return 1; }
    kosk_set_entropy(h, KOSK_ENTROPY_SEED);
    const int D = kosk_registry_tree_depth(n);
    const size_t rec = kosk_regsort_proof_bytes(D);
    std::vector<uint8_t> pk(n * pkb), sk(n * skb), pi(n * pib), proven(n), ok(n), status(n), kind(n), state(1);
    std::vector<uint8_t> fp(n * 32), records((size_t)n * rec), old(rec), path((size_t)D * 32 + 1), stored(32);
    std::vector<uint8_t> root(32), root2(32), slot_root(32), got(32);
    std::vector<int32_t> slots(n);
    int all = 1;
    auto stage = [&](const char *what, bool good) {
        printf("[registry_absent] kyber_k %d, %d peers: %s = %d\n", k, n, what, (int)good);
        all &= (int)good;
    };

    MUST(kosk_kem_keypair_batch(h, n, nullptr, pk.data(), sk.data()));
    MUST(kosk_prove_keys_batch(h, n, sk.data(), nullptr, 0, pi.data(), proven.data()));
    MUST(kosk_verify_batch(h, n, pi.data(), pk.data(), ok.data()));
    int used = -1, cap = -1, good = 0;
    MUST(kosk_registry_reserve(h, n));
    MUST(kosk_registry_enrol_verified(h, n, slots.data(), status.data()));
    MUST(kosk_registry_level(h, &used, &cap));
    for (int b = 0; b < n; b++) good += proven[b] == 1 && ok[b] == 1 && status[b] == KOSK_ENROL_ADMITTED;
    stage("kosk_verify_batch + kosk_registry_enrol_verified: every key proven and enrolled", good == n && used == n && cap == n);

    // a fingerprint nobody enrolled: the hash of something that is no key of this registry
    for (int b = 0; b < n; b++) kosk_host_sha3_256(&fp[b * 32], &pk[b * pkb], pkb);
    uint8_t unknown[32];
    kosk_host_sha3_256(unknown, fp.data(), fp.size());
    MUST(kosk_registry_sorted_root(h, root.data(), &used, &cap));
    MUST(kosk_registry_prove_absent(h, 1, unknown, kind.data(), old.data(), root2.data()));
    stage("kosk_registry_sorted_root + kosk_registry_prove_absent: an unknown fingerprint is proven absent on the host",
          used == n && cap == n && !memcmp(root.data(), root2.data(), 32) && kind[0] == 1 &&
              kosk_regsort_check_proof(k, D, unknown, old.data(), root.data()) == 1);

    // every enrolled key is PRESENT, and the slot its record names holds the same fingerprint in the slot tree
    MUST(kosk_registry_prove_absent(h, n, fp.data(), kind.data(), records.data(), nullptr));
    MUST(kosk_registry_root(h, slot_root.data(), nullptr, nullptr));
    bool linked = true;
    for (int b = 0; b < n; b++) {
        const uint8_t *r = &records[(size_t)b * rec];
        int32_t slot;
        memcpy(&slot, r + 4, 4); // slot_l; the example runs on a little-endian host
        linked = linked && kind[b] == 2 && kosk_regsort_check_proof(k, D, &fp[b * 32], r, root.data()) == 2 && slot == slots[b];
        MUST(kosk_registry_prove_slots(h, 1, &slot, state.data(), stored.data(), path.data(), nullptr));
        linked = linked && state[0] == 1 && !memcmp(stored.data(), &fp[b * 32], 32) &&
                 kosk_regtree_root_from_path(k, D, slot, &fp[b * 32], path.data(), got.data()) == 0 && !memcmp(got.data(), slot_root.data(), 32);
    }
    stage("an enrolled fingerprint is PRESENT, and its slot's path leads to the slot tree's root", linked);

    std::vector<uint8_t> bent(old);
    bent[16 + 7] ^= 0x40; // h_l, or zeros where there is no left record: the walk or the flags' promise breaks either way
    bent[80 + (size_t)D * 32 + 3] ^= 0x01;
    stage("one flipped byte in each half of the proof: it proves neither", kosk_regsort_check_proof(k, D, unknown, bent.data(), root.data()) == 0);

    const int victim = 2;
    const int32_t gone = slots[victim];
    MUST(kosk_registry_evict(h, 1, &gone));
    MUST(kosk_registry_prove_absent(h, 1, &fp[victim * 32], kind.data(), records.data(), root2.data()));
    stage("kosk_registry_evict: under the new root the key is absent, and the old record no longer checks",
          memcmp(root.data(), root2.data(), 32) != 0 && kind[0] == 1 && kosk_regsort_check_proof(k, D, &fp[victim * 32], records.data(), root2.data()) == 1 &&
              kosk_regsort_check_proof(k, D, unknown, old.data(), root2.data()) == 0);

    kosk_destroy(h);
    printf("[result] registry_absent success = %d\n", all);
    return all ? 0 : 1;
}
