// Signed heads on the C ABI (include/kosk_mi355x.h): the trust chain of 8.9 from a public key to an encapsulation with
// nothing taken from outside this library.
//   1. a registrar reserves a signer, enrols half its peers, checkpoints   kosk_registry_signer_reserve, kosk_registry_enrol,
//      and signs the head; enrols the rest, checkpoints and signs again    kosk_registry_history_checkpoint, kosk_registry_history_sign_head
//   2. a gateway that knows only the public key verifies both signatures   kosk_headsig_verify
//      on the host, and both in one batch on the GPU                        kosk_headsig_verify_heads
//   3. it checks that the second head extends the first                    kosk_registry_history_prove_consistency, kosk_reghist_check_consistency
//   4. it checks the second checkpoint's inclusion under the second head   kosk_reghist_leaf, kosk_reghist_root_from_path
//   5. it encapsulates to the peers proven under that checkpoint's root     kosk_kem_enc_proven
//   6. the peers decapsulate to equal secrets                               kosk_kem_dec_batch
//   7. a flipped byte in a signature is rejected
//   8. the same head signed under another seed is rejected
// One line per stage and one for the result, each ending in "= 1" where it holds.
//   registry_signed [kyber_k = 3] [n = 8]
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
    const int height = 10; // 1 024 heads: the history below holds n + 2 events
    if (k < 2 || k > 4 || n < 4 || n > 1000) { fprintf(stderr, "usage: registry_signed [2|3|4] [4 <= n <= 1000]\n"); return 2; }
    const size_t pkb = kosk_pk_bytes(k), skb = kosk_sk_bytes(k), ctb = kosk_ct_bytes(k), E = KOSK_REGHIST_EVENT_BYTES, sb = kosk_headsig_sig_bytes(height);
    kosk_ctx *h = nullptr, *g = nullptr; // the registrar, the gateway
    if (kosk_create(&h, 0, k, n) || kosk_create(&g, 0, k, 1)) { fprintf(stderr, "kosk_create: %s\n", kosk_last_error(nullptr)); return 1; }
    int all = 1;
    auto stage = [&](const char *what, bool good) {
        printf("[registry_signed] kyber_k %d, %d peers: %s = %d\n", k, n, what, (int)good);
        all &= (int)good;
    };

    // 1. the registrar.  One seed serves one history: this seed is never used for another log
    uint8_t seed[32], other_seed[32], id[16], pub[KOSK_HEADSIG_PUB_BYTES];
    for (int i = 0; i < 32; i++) { seed[i] = (uint8_t)(0xC3 ^ (7 * i)); other_seed[i] = (uint8_t)(0x3C ^ (5 * i)); }
    for (int i = 0; i < 16; i++) id[i] = (uint8_t)('a' + i);
    const int half = n / 2;
    std::vector<uint8_t> pk(n * pkb), sk(n * skb), status(n), roots(2 * 32), sigs(2 * sb);
    std::vector<int32_t> slots(n);
    int32_t sizes[2] = {-1, -1};
    int cp = -1, admitted = 0, s = -1, has_seed = 0, lvl = 0;
    MUST(kosk_kem_keypair_batch(h, n, nullptr, pk.data(), sk.data()));
    MUST(kosk_registry_reserve(h, n));
    MUST(kosk_registry_history_reserve(h, n + 2));
    MUST(kosk_registry_signer_reserve(h, height, seed, id, pub));
    MUST(kosk_registry_signer_level(h, &lvl, &has_seed));
    MUST(kosk_registry_enrol(h, half, pk.data(), nullptr, slots.data(), status.data()));
    MUST(kosk_registry_history_checkpoint(h, &cp));
    MUST(kosk_registry_history_sign_head(h, -1, &sigs[0], &roots[0], &s));
    sizes[0] = s;
    MUST(kosk_registry_enrol(h, n - half, &pk[half * pkb], nullptr, &slots[half], &status[half]));
    MUST(kosk_registry_history_checkpoint(h, &cp));
    MUST(kosk_registry_history_sign_head(h, -1, &sigs[sb], &roots[32], &s));
    sizes[1] = s;
    for (int b = 0; b < n; b++) admitted += status[b] == KOSK_ENROL_ADMITTED;
    stage("a registrar enrols, checkpoints and signs two heads",
          admitted == n && lvl == height && has_seed == 1 && sizes[0] == half + 1 && sizes[1] == n + 2 && cp == n + 1 && le32(pub) == (uint32_t)height);

    // 2. the gateway knows pub and nothing else: no registry, no history, no signer
    uint8_t ok[2] = {0, 0};
    MUST(kosk_headsig_verify_heads(g, 2, pub, roots.data(), sizes, sigs.data(), ok));
    stage("the gateway verifies both signatures on the host and in one batch on the GPU",
          kosk_headsig_verify(pub, k, &roots[0], sizes[0], &sigs[0]) == 1 && kosk_headsig_verify(pub, k, &roots[32], sizes[1], &sigs[sb]) == 1 && ok[0] == 1 && ok[1] == 1);

    // 3. the second head extends the first
    std::vector<uint8_t> cons(kosk_reghist_consistency_bytes(sizes[1]));
    const int32_t old_size = sizes[0];
    MUST(kosk_registry_history_prove_consistency(h, sizes[1], 1, &old_size, cons.data(), nullptr));
    stage("the second head extends the first", kosk_reghist_check_consistency(sizes[0], sizes[1], &roots[0], &roots[32], cons.data()) == 1);

    // 4. the second checkpoint lies under the second head
    std::vector<uint8_t> event(E), leaf(32), evleaf(32), got(32), incl(kosk_reghist_path_bytes(sizes[1]) + 1);
    const int32_t index = cp;
    MUST(kosk_registry_history_read(h, cp, 1, event.data()));
    MUST(kosk_registry_history_prove_events(h, sizes[1], 1, &index, leaf.data(), incl.data(), nullptr));
    stage("the checkpoint's inclusion under the signed head holds on the host",
          le32(event.data()) == KOSK_REGHIST_CHECKPOINT && kosk_reghist_leaf(k, event.data(), evleaf.data()) == 0 && !memcmp(evleaf.data(), leaf.data(), 32) &&
              kosk_reghist_root_from_path(cp, sizes[1], evleaf.data(), incl.data(), got.data()) == 0 && !memcmp(got.data(), &roots[32], 32));

    // 5. as registry_relying goes on: encapsulate to the keys proven under the checkpoint's slot_root
    const int D = kosk_registry_tree_depth(n);
    const uint8_t *slot_root = &event[16];
    std::vector<uint8_t> state(n), paths((size_t)n * D * 32 + 1), sent_paths, ct(n * ctb), ss(n * 32), ss2(n * 32), done(n);
    MUST(kosk_registry_prove_slots(h, n, slots.data(), state.data(), nullptr, paths.data(), nullptr));
    sent_paths = paths;
    const int tampered = 1;
    if (D > 0) sent_paths[(size_t)tampered * D * 32 + 5] ^= 0x40;
    MUST(kosk_kem_enc_proven(g, n, D, pk.data(), slots.data(), sent_paths.data(), slot_root, nullptr, ct.data(), ss.data(), done.data()));
    bool verdicts = true;
    for (int b = 0; b < n; b++) verdicts = verdicts && done[b] == (D == 0 || b != tampered);
    stage("kosk_kem_enc_proven: every key but the tampered one is proven under the signed head's checkpoint", verdicts);

    // 6. the peers decapsulate
    MUST(kosk_kem_dec_batch(h, n, ct.data(), sk.data(), ss2.data()));
    bool equal = true;
    for (int b = 0; b < n; b++)
        if (done[b]) equal = equal && !memcmp(&ss[(size_t)b * 32], &ss2[(size_t)b * 32], 32);
    stage("the accepted peers decapsulate to the gateway's shared secrets", equal);

    // 7. one flipped byte anywhere in a signature
    bool rejected = true;
    for (size_t at : {(size_t)5, (size_t)20, (size_t)48 + 32 * 17 + 3, sb - 1}) {
        std::vector<uint8_t> bad(sigs.begin() + sb, sigs.end());
        bad[at] ^= 0x01;
        uint8_t v = 9;
        MUST(kosk_headsig_verify_heads(g, 1, pub, &roots[32], &sizes[1], bad.data(), &v));
        rejected = rejected && v == 0 && kosk_headsig_verify(pub, k, &roots[32], sizes[1], bad.data()) == 0;
    }
    stage("a flipped byte in a signature is rejected", rejected);

    // 8. another seed is another key: its signature of the same head does not verify under pub
    uint8_t other_pub[KOSK_HEADSIG_PUB_BYTES], v = 9;
    std::vector<uint8_t> other_sig(sb), other_root(32);
    MUST(kosk_registry_signer_reserve(h, height, other_seed, id, other_pub));
    MUST(kosk_registry_history_sign_head(h, sizes[1], other_sig.data(), other_root.data(), nullptr));
    MUST(kosk_headsig_verify_heads(g, 1, pub, &roots[32], &sizes[1], other_sig.data(), &v));
    stage("the same head signed under another seed is rejected",
          !memcmp(other_root.data(), &roots[32], 32) && memcmp(other_pub, pub, sizeof pub) != 0 && v == 0 &&
              kosk_headsig_verify(pub, k, &roots[32], sizes[1], other_sig.data()) == 0 && kosk_headsig_verify(other_pub, k, &roots[32], sizes[1], other_sig.data()) == 1);

    kosk_destroy(g);
    kosk_destroy(h);
    printf("[result] registry_signed success = %d\n", all);
    return all ? 0 : 1;
}
