// The registry history on the C ABI (include/kosk_mi355x.h, INTEGRATION.md 8.7, format kosk-reghist-v1): a registrar whose peers can check
// that every head it publishes extends the one before -- no key evicted and enrolled again behind their backs, no second table.
//   1. n ordinary key pairs; the registrar reserves a history, enrols     kosk_kem_keypair_batch, kosk_registry_history_reserve,
//      the first half and publishes a head                                kosk_registry_enrol, kosk_registry_history_head
//   2. it enrols the rest, a peer leaves, a checkpoint binds both         kosk_registry_evict, kosk_registry_history_checkpoint,
//      state roots into the log; a second head                            kosk_registry_history_head
//   3. the consistency proof between the two heads checks on the host     kosk_registry_history_prove_consistency, kosk_reghist_check_consistency
//   4. the checkpoint event is in the log under the second head           kosk_registry_history_read, kosk_reghist_leaf,
//                                                                         kosk_registry_history_prove_events, kosk_reghist_root_from_path
//   5. its slot_root is kosk_registry_root, and an auditor who replays    kosk_registry_root, kosk_regtree_leaf, kosk_regtree_node
//      the events onto an empty table recomputes it on the host
//   6. a forked old head is rejected                                      kosk_reghist_check_consistency
// One line per stage and one for the result, each ending in "= 1" where it holds.
//   registry_history [kyber_k = 3] [n = 8]
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

static uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

int main(int argc, char **argv)
{
    const int k = argc > 1 ? atoi(argv[1]) : 3;
    const int n = argc > 2 ? atoi(argv[2]) : 8;
    if (k < 2 || k > 4 || n < 4) { fprintf(stderr, "usage: registry_history [2|3|4] [n >= 4]\n"); return 2; }
    const size_t pkb = kosk_pk_bytes(k), skb = kosk_sk_bytes(k);
    kosk_ctx *h = nullptr;
    if (kosk_create(&h, 0, k, n)) { fprintf(stderr, "kosk_create: %s\n", kosk_last_error(nullptr)); return 1; }
    std::vector<uint8_t> pk(n * pkb), sk(n * skb), status(n), head1(32), head2(32), root(32), leaf(32), got(32), slot_root(32);
    std::vector<int32_t> slots(n);
    int all = 1;
    auto stage = [&](const char *what, bool good) {
        printf("[registry_history] kyber_k %d, %d peers: %s = %d\n", k, n, what, (int)good);
        all &= (int)good;
    };

    const int first = n / 2, max_events = 2 * n + 2;
    int size1 = -1, size2 = -1, level = -1, cap = -1, good = 0;
    MUST(kosk_kem_keypair_batch(h, n, nullptr, pk.data(), sk.data()));
    MUST(kosk_registry_reserve(h, n));
    MUST(kosk_registry_history_reserve(h, max_events));
    MUST(kosk_registry_enrol(h, first, pk.data(), nullptr, slots.data(), status.data()));
    for (int b = 0; b < first; b++) good += status[b] == KOSK_ENROL_ADMITTED;
    MUST(kosk_registry_history_head(h, -1, head1.data(), &size1));
    stage("kosk_registry_history_reserve + kosk_registry_enrol: one event per key, a first head", good == first && size1 == first);

    const int32_t gone = slots[1];
    int cp = -1;
    MUST(kosk_registry_enrol(h, n - first, &pk[first * pkb], nullptr, &slots[first], &status[first]));
    MUST(kosk_registry_evict(h, 1, &gone));
    MUST(kosk_registry_history_checkpoint(h, &cp));
    MUST(kosk_registry_history_head(h, -1, head2.data(), &size2));
    MUST(kosk_registry_history_level(h, &level, &cap));
    stage("enrol, evict, kosk_registry_history_checkpoint: a second head", size2 == n + 2 && cp == n + 1 && level == size2 && cap == max_events &&
              memcmp(head1.data(), head2.data(), 32) != 0);

    std::vector<uint8_t> cons(kosk_reghist_consistency_bytes(size2));
    const int32_t old_size = size1;
    MUST(kosk_registry_history_prove_consistency(h, size2, 1, &old_size, cons.data(), root.data()));
    stage("kosk_registry_history_prove_consistency: the second head extends the first, checked on the host",
          !memcmp(root.data(), head2.data(), 32) && kosk_reghist_check_consistency(size1, size2, head1.data(), head2.data(), cons.data()) == 1);

    std::vector<uint8_t> events((size_t)size2 * KOSK_REGHIST_EVENT_BYTES), incl(kosk_reghist_path_bytes(size2));
    const uint8_t *ev = &events[(size_t)cp * KOSK_REGHIST_EVENT_BYTES];
    const int32_t index = cp;
    MUST(kosk_registry_history_read(h, 0, size2, events.data()));
    MUST(kosk_registry_history_prove_events(h, size2, 1, &index, leaf.data(), incl.data(), nullptr));
    stage("kosk_registry_history_prove_events: the checkpoint event is in the log under the second head",
          le32(ev) == KOSK_REGHIST_CHECKPOINT && kosk_reghist_leaf(k, ev, got.data()) == 0 && !memcmp(got.data(), leaf.data(), 32) &&
              kosk_reghist_root_from_path(cp, size2, leaf.data(), incl.data(), got.data()) == 0 && !memcmp(got.data(), head2.data(), 32));

    // the auditor: replay the events onto an empty table, then the slot tree of kosk-regtree-v1 over it
    const int D = kosk_registry_tree_depth(n), P = 1 << D;
    std::vector<uint8_t> table((size_t)n * 32), occupied(n, 0), lv((size_t)P * 32);
    bool replayed = true;
    for (int e = 0; e < size2; e++) {
        const uint8_t *r = &events[(size_t)e * KOSK_REGHIST_EVENT_BYTES];
        const uint32_t op = le32(r), slot = le32(r + 4);
        if (op == KOSK_REGHIST_CHECKPOINT) continue;
        replayed = replayed && slot < (uint32_t)n && occupied[slot] == (op == KOSK_REGHIST_EVICT) && (op != KOSK_REGHIST_EVICT || !memcmp(&table[slot * 32], r + 16, 32));
        if (!replayed) break;
        occupied[slot] = op == KOSK_REGHIST_ADMIT;
        memcpy(&table[slot * 32], r + 16, 32);
    }
    int used = 0;
    for (int s = 0; s < P; s++) {
        used += s < n && occupied[s];
        replayed = replayed && kosk_regtree_leaf(k, s < n && occupied[s] ? &table[(size_t)s * 32] : nullptr, &lv[(size_t)s * 32]) == 0;
    }
    for (int w = P; w > 1; w /= 2)
        for (int i = 0; i < w / 2; i++) replayed = replayed && kosk_regtree_node(&lv[(size_t)2 * i * 32], &lv[(size_t)(2 * i + 1) * 32], &lv[(size_t)i * 32]) == 0;
    MUST(kosk_registry_root(h, slot_root.data(), nullptr, nullptr));
    stage("the checkpoint's slot_root is kosk_registry_root and the root an auditor recomputes from the replayed events",
          replayed && !memcmp(ev + 16, slot_root.data(), 32) && !memcmp(ev + 16, lv.data(), 32) && le32(ev + 4) == (uint32_t)used && used == n - 1 &&
              le32(ev + 8) == (uint32_t)n);

    std::vector<uint8_t> forked(head1);
    forked[0] ^= 1;
    stage("a forked old head is rejected", kosk_reghist_check_consistency(size1, size2, forked.data(), head2.data(), cons.data()) == 0);

    kosk_destroy(h);
    printf("[result] registry_history success = %d\n", all);
    return all ? 0 : 1;
}
