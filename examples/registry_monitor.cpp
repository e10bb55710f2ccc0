// The registry monitor on the C ABI (include/kosk_mi355x.h): the third role of the transparency log.  A monitor replays
// the registrar's whole event log and checks that every checkpoint's roots are the roots of what the events produce.
//   1. a registrar enrols n key pairs, a peer leaves, a checkpoint;      kosk_registry_enrol, kosk_registry_evict,
//      it enrols a latecomer into the free slot, a second checkpoint      kosk_registry_history_checkpoint
//   2. a monitor on a second handle is fed the log in two instalments;    kosk_registry_history_read, kosk_monitor_reserve, kosk_monitor_feed,
//      after each, the head and both roots are the registrar's            kosk_monitor_head, kosk_monitor_roots, kosk_monitor_level
//   3. the replayed table is the registrar's                              kosk_monitor_read, kosk_registry_read
//   4. a copy of the log with one flipped bit in a checkpoint's           kosk_monitor_feed: KOSK_MONITOR_CP_SORTED_ROOT
//      sorted_root is rejected at that index; the monitor has failed
//   5. a log with an evict of the wrong fingerprint is rejected           kosk_monitor_feed: KOSK_MONITOR_EVICT_MISMATCH
// One line per stage and one for the result, each ending in "= 1" where it holds.
//   registry_monitor [kyber_k = 3] [n = 8]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kosk_mi355x.h"

#define MUST(x)                                                                       \
    do {                                                                              \
        if ((x) < 0) {                                                                \
            fprintf(stderr, "%s: %s / %s\n", #x, kosk_last_error(h), kosk_last_error(m)); \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

static uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

int main(int argc, char **argv)
{
    const int k = argc > 1 ? atoi(argv[1]) : 3;
    const int n = argc > 2 ? atoi(argv[2]) : 8;
    if (k < 2 || k > 4 || n < 4) { fprintf(stderr, "usage: registry_monitor [2|3|4] [n >= 4]\n"); return 2; }
    const size_t pkb = kosk_pk_bytes(k), skb = kosk_sk_bytes(k), E = KOSK_REGHIST_EVENT_BYTES;
    kosk_ctx *h = nullptr, *m = nullptr;
    if (kosk_create(&h, 0, k, n + 1) || kosk_create(&m, 0, k, 1)) { fprintf(stderr, "kosk_create: %s\n", kosk_last_error(nullptr)); return 1; }
    std::vector<uint8_t> pk((n + 1) * pkb), sk((n + 1) * skb), status(n + 1);
    std::vector<int32_t> slots(n + 1);
    int all = 1;
    auto stage = [&](const char *what, bool good) {
        printf("[registry_monitor] kyber_k %d, %d peers: %s = %d\n", k, n, what, (int)good);
        all &= (int)good;
    };

    // 1. the registrar
    const int max_events = n + 4;
    int cp1 = -1, cp2 = -1, size = -1;
    MUST(kosk_kem_keypair_batch(h, n + 1, nullptr, pk.data(), sk.data()));
    MUST(kosk_registry_reserve(h, n));
    MUST(kosk_registry_history_reserve(h, max_events));
    MUST(kosk_registry_enrol(h, n, pk.data(), nullptr, slots.data(), status.data()));
    const int32_t gone = slots[1];
    MUST(kosk_registry_evict(h, 1, &gone));
    MUST(kosk_registry_history_checkpoint(h, &cp1));
    MUST(kosk_registry_enrol(h, 1, &pk[n * pkb], nullptr, &slots[n], &status[n]));
    MUST(kosk_registry_history_checkpoint(h, &cp2));
    MUST(kosk_registry_history_level(h, &size, nullptr));
    stage("a registrar enrols, evicts, checkpoints, enrols a latecomer and checkpoints again", cp1 == n + 1 && cp2 == n + 3 && size == n + 4 && slots[n] == gone);

    // 2. the monitor, in two instalments: up to the first checkpoint, then the rest
    std::vector<uint8_t> log((size_t)size * E), head(32), mhead(32), sroot(32), troot(32), msroot(32), mtroot(32);
    MUST(kosk_registry_history_read(h, 0, size, log.data()));
    MUST(kosk_monitor_reserve(m, n, max_events));
    bool fed = true;
    const int cut[3] = {0, cp1 + 1, size};
    for (int part = 0; part < 2; part++) {
        int bad = 0, why = -1, msize = -1, mused = -1, failed = -1, at = -1;
        fed = fed && kosk_monitor_feed(m, cut[part + 1] - cut[part], &log[(size_t)cut[part] * E], &bad, &why) == 1 && bad == -1 && why == KOSK_MONITOR_OK;
        MUST(kosk_monitor_level(m, &msize, nullptr, &mused, nullptr, &failed));
        MUST(kosk_monitor_head(m, -1, mhead.data(), &at));
        MUST(kosk_registry_history_head(h, cut[part + 1], head.data(), nullptr));
        fed = fed && msize == cut[part + 1] && at == msize && !failed && !memcmp(head.data(), mhead.data(), 32);
        // the checkpoint that ends the instalment holds the registrar's roots at that time; the monitor's are those of its replayed table
        const uint8_t *cp = &log[(size_t)(cut[part + 1] - 1) * E];
        MUST(kosk_monitor_roots(m, mtroot.data(), msroot.data()));
        fed = fed && le32(cp) == KOSK_REGHIST_CHECKPOINT && le32(cp + 4) == (uint32_t)mused && !memcmp(cp + 16, mtroot.data(), 32) && !memcmp(cp + 48, msroot.data(), 32);
    }
    MUST(kosk_registry_root(h, troot.data(), nullptr, nullptr));
    MUST(kosk_registry_sorted_root(h, sroot.data(), nullptr, nullptr));
    stage("kosk_monitor_feed in two instalments: the heads and both roots are the registrar's", fed && !memcmp(troot.data(), mtroot.data(), 32) && !memcmp(sroot.data(), msroot.data(), 32));

    // 3. the table
    std::vector<int32_t> every(n);
    for (int s = 0; s < n; s++) every[s] = s;
    std::vector<uint8_t> st(n), mst(n), fp((size_t)n * 32), mfp((size_t)n * 32);
    MUST(kosk_registry_read(h, n, every.data(), st.data(), nullptr, fp.data()));
    MUST(kosk_monitor_read(m, n, every.data(), mst.data(), mfp.data()));
    stage("kosk_monitor_read: the replayed table is the registrar's, slot by slot", st == mst && fp == mfp);

    // 4. one flipped bit in the second checkpoint's sorted_root
    std::vector<uint8_t> forged(log);
    forged[(size_t)cp2 * E + 48 + 7] ^= 0x10;
    int bad = -1, why = -1, msize = -1, failed = -1, extra = -1;
    MUST(kosk_monitor_reserve(m, n, max_events));
    const int rc = kosk_monitor_feed(m, size, forged.data(), &bad, &why);
    MUST(kosk_monitor_level(m, &msize, nullptr, nullptr, nullptr, &failed));
    MUST(kosk_monitor_head(m, -1, mhead.data(), nullptr));
    MUST(kosk_registry_history_head(h, msize, head.data(), nullptr));
    extra = kosk_monitor_feed(m, 1, forged.data(), nullptr, nullptr);
    stage("a flipped bit in a checkpoint's sorted_root is rejected at that index: KOSK_MONITOR_CP_SORTED_ROOT, and the monitor has failed",
          rc == 0 && bad == cp2 && why == KOSK_MONITOR_CP_SORTED_ROOT && failed == 1 && msize <= bad && !memcmp(head.data(), mhead.data(), 32) && extra == -1);

    // 5. an evict of the wrong fingerprint: the registrar's EVICT event with the fingerprint of another peer
    forged = log;
    memcpy(&forged[(size_t)n * E + 16], &log[16], 32);
    bad = why = -1;
    MUST(kosk_monitor_reserve(m, n, max_events));
    const int rc2 = kosk_monitor_feed(m, size, forged.data(), &bad, &why);
    stage("an evict of the wrong fingerprint is rejected: KOSK_MONITOR_EVICT_MISMATCH",
          le32(&log[(size_t)n * E]) == KOSK_REGHIST_EVICT && gone != (int32_t)le32(&log[4]) && rc2 == 0 && bad == n && why == KOSK_MONITOR_EVICT_MISMATCH);

    kosk_destroy(m);
    kosk_destroy(h);
    printf("[result] registry_monitor success = %d\n", all);
    return all ? 0 : 1;
}
