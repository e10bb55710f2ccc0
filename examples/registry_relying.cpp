// The relying party on the C ABI (include/kosk_mi355x.h): the role the transparency log exists for.  A gateway that holds
// a signed head receives peers' public keys with their proofs and encapsulates only to keys that are really enrolled.
//   1. a registrar enrols n key pairs, checkpoints, and hands out a head,   kosk_registry_enrol, kosk_registry_history_checkpoint,
//      the checkpoint event with its inclusion record, and per key          kosk_registry_history_head, kosk_registry_history_prove_events,
//      (pk, slot, path)                                                     kosk_registry_prove_slots
//   2. a second handle with NO registry checks the checkpoint's inclusion   kosk_reghist_leaf, kosk_reghist_root_from_path
//      under the head, on the host
//   3. it takes slot_root and sorted_root from the event
//   4. it encapsulates to the peers in one call, one tampered path and      kosk_kem_enc_proven
//      one substituted pk among the items
//   5. the peers decapsulate the accepted items to equal secrets            kosk_kem_dec_batch
//   6. the two bad items have done = 0 and zero ct and ss
//   7. an absence proof for a fresh fingerprint and a presence proof for    kosk_registry_prove_absent, kosk_regsort_check_proofs
//      an enrolled one check under sorted_root
// One line per stage and one for the result, each ending in "= 1" where it holds.
//   registry_relying [kyber_k = 3] [n = 8]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kosk_mi355x.h"

#define MUST(x)                                                                       \
    do {                                                                              \
        if ((x) < 0) {                                                                \
            fprintf(stderr, "%s: %s / %s\n", #x, kosk_last_error(h), kosk_last_error(g)); \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

static uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

int main(int argc, char **argv)
{
    const int k = argc > 1 ? atoi(argv[1]) : 3;
    const int n = argc > 2 ? atoi(argv[2]) : 8;
    if (k < 2 || k > 4 || n < 4) { fprintf(stderr, "usage: registry_relying [2|3|4] [n >= 4]\n"); return 2; }
    const size_t pkb = kosk_pk_bytes(k), skb = kosk_sk_bytes(k), ctb = kosk_ct_bytes(k), E = KOSK_REGHIST_EVENT_BYTES;
    kosk_ctx *h = nullptr, *g = nullptr; // the registrar, the gateway
    if (kosk_create(&h, 0, k, n) || kosk_create(&g, 0, k, 1)) { fprintf(stderr, "kosk_create: %s\n", kosk_last_error(nullptr)); return 1; }
    int all = 1;
    auto stage = [&](const char *what, bool good) {
        printf("[registry_relying] kyber_k %d, %d peers: %s = %d\n", k, n, what, (int)good);
        all &= (int)good;
    };

    // 1. the registrar
    const int D = kosk_registry_tree_depth(n);
    std::vector<uint8_t> pk(n * pkb), sk(n * skb), status(n), state(n), head(32), paths((size_t)n * D * 32 + 1);
    std::vector<int32_t> slots(n);
    int cp = -1, size = -1, admitted = 0;
    MUST(kosk_kem_keypair_batch(h, n, nullptr, pk.data(), sk.data()));
    MUST(kosk_registry_reserve(h, n));
    MUST(kosk_registry_history_reserve(h, n + 1));
    MUST(kosk_registry_enrol(h, n, pk.data(), nullptr, slots.data(), status.data()));
    for (int b = 0; b < n; b++) admitted += status[b] == KOSK_ENROL_ADMITTED;
    MUST(kosk_registry_history_checkpoint(h, &cp));
    MUST(kosk_registry_history_head(h, -1, head.data(), &size));
    std::vector<uint8_t> event(E), leaf(32), incl(kosk_reghist_path_bytes(size) + 1);
    const int32_t index = cp;
    MUST(kosk_registry_history_read(h, cp, 1, event.data()));
    MUST(kosk_registry_history_prove_events(h, size, 1, &index, leaf.data(), incl.data(), nullptr));
    MUST(kosk_registry_prove_slots(h, n, slots.data(), state.data(), nullptr, paths.data(), nullptr));
    stage("a registrar enrols, checkpoints and hands out a head, the checkpoint's record and per key (pk, slot, path)", admitted == n && cp == n && size == n + 1);

    // 2. the gateway: no registry, no history, no monitor.  The head is what it trusts (its signature is out of scope here)
    std::vector<uint8_t> got(32), evleaf(32);
    int used = -1, capacity = -1;
    MUST(kosk_registry_level(g, &used, &capacity));
    stage("the gateway checks the checkpoint's inclusion under the head on the host",
          used == 0 && capacity == 0 && le32(event.data()) == KOSK_REGHIST_CHECKPOINT && kosk_reghist_leaf(k, event.data(), evleaf.data()) == 0 &&
              !memcmp(evleaf.data(), leaf.data(), 32) && kosk_reghist_root_from_path(cp, size, evleaf.data(), incl.data(), got.data()) == 0 && !memcmp(got.data(), head.data(), 32));

    // 3. the two state roots the checkpoint binds
    const uint8_t *slot_root = &event[16], *sorted_root = &event[48];
    std::vector<uint8_t> troot(32), sroot(32);
    MUST(kosk_registry_root(h, troot.data(), nullptr, nullptr));
    MUST(kosk_registry_sorted_root(h, sroot.data(), nullptr, nullptr));
    stage("slot_root and sorted_root come from the event", le32(&event[4]) == (uint32_t)n && !memcmp(slot_root, troot.data(), 32) && !memcmp(sorted_root, sroot.data(), 32));

    // 4. one call: fingerprint, check, encapsulate.  Peer 1 sends a tampered path, peer 2's key was substituted on the way
    std::vector<uint8_t> sent(pk), sent_paths(paths), ct(n * ctb), ss(n * 32), done(n);
    const int tampered = 1, substituted = 2;
    if (D > 0) sent_paths[(size_t)tampered * D * 32 + 5] ^= 0x40;
    else sent[(size_t)tampered * pkb + 9] ^= 0x40; // a tree of one slot has no path to tamper with
    memcpy(&sent[(size_t)substituted * pkb], &pk[0], pkb);
    MUST(kosk_kem_enc_proven(g, n, D, sent.data(), slots.data(), sent_paths.data(), slot_root, nullptr, ct.data(), ss.data(), done.data()));
    bool verdicts = true;
    for (int b = 0; b < n; b++) verdicts = verdicts && done[b] == (b != tampered && b != substituted);
    stage("kosk_kem_enc_proven: every key but the two bad ones is proven under slot_root", verdicts);

    // 5. the peers decapsulate
    std::vector<uint8_t> ss2(n * 32);
    MUST(kosk_kem_dec_batch(h, n, ct.data(), sk.data(), ss2.data()));
    bool equal = true;
    for (int b = 0; b < n; b++)
        if (done[b]) equal = equal && !memcmp(&ss[(size_t)b * 32], &ss2[(size_t)b * 32], 32);
    stage("the accepted peers decapsulate to the gateway's shared secrets", equal);

    // 6. nothing was made for the bad ones
    bool zero = true;
    for (int b : {tampered, substituted}) {
        for (size_t i = 0; i < ctb; i++) zero = zero && ct[(size_t)b * ctb + i] == 0;
        for (size_t i = 0; i < 32; i++) zero = zero && ss[(size_t)b * 32 + i] == 0;
    }
    stage("the two bad items have done = 0 and zero ct and ss", zero && !done[tampered] && !done[substituted]);

    // 7. absence and presence under sorted_root
    const size_t rec = kosk_regsort_proof_bytes(D);
    std::vector<uint8_t> x(64), kind(2), records(2 * rec), verdict(2), fps((size_t)n * 32);
    MUST(kosk_registry_read(h, n, slots.data(), state.data(), nullptr, fps.data()));
    memcpy(&x[0], &fps[0], 32);
    for (int i = 0; i < 32; i++) x[32 + i] = (uint8_t)(fps[i] ^ 0x5a); // a fingerprint nobody has
    MUST(kosk_registry_prove_absent(h, 2, x.data(), kind.data(), records.data(), nullptr));
    MUST(kosk_regsort_check_proofs(g, 2, D, x.data(), records.data(), sorted_root, verdict.data()));
    stage("kosk_regsort_check_proofs: PRESENT for an enrolled fingerprint, ABSENT for a fresh one",
          kind[0] == 2 && kind[1] == 1 && verdict[0] == 2 && verdict[1] == 1 &&
              kosk_regsort_check_proof(k, D, &x[32], &records[rec], sorted_root) == 1);

    kosk_destroy(g);
    kosk_destroy(h);
    printf("[result] registry_relying success = %d\n", all);
    return all ? 0 : 1;
}
