// Enrolment with context-bound proofs of possession (format kosk-bind-v1) on the C ABI, end to end:
//   1. N clients hold Kyber key pairs that already exist                      kosk_keygen (host; any Kyber implementation's keys do)
//   2. the registrar hands every client a fresh nonce; both sides compute     context_b = SHA3-256(identity_b || nonce_b)
//   3. the clients prove knowledge of their secret keys UNDER their contexts  kosk_set_contexts + kosk_prove_keys_batch
//   4. the registrar verifies under the contexts it issued                    kosk_set_contexts + kosk_verify_batch
//   5. and encapsulates to the keys it accepted, in HBM                       kosk_kem_enc_verified
//   6. the clients decapsulate; both sides hold the same shared secrets       kosk_kem_dec_batch
//   7. the same (pk, proof) pairs presented again under NEW nonces -- a replay -- are all rejected, and so are they on a handle that
//      is not armed at all
//   enrol_bound [kyber_k = 3] [n = 4]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "kosk_mi355x.h"

static std::mt19937_64 g_rng(20260202); // a deterministic stand-in: this is an example, not a key generator
static void fill(uint8_t *out, size_t len)
{
    for (size_t i = 0; i < len; i++) out[i] = (uint8_t)g_rng();
}

#define MUST(x)                                                                       \
    do {                                                                              \
        if (x) {                                                                      \
            fprintf(stderr, "%s: %s\n", #x, kosk_last_error(h));                      \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

// context_b = SHA3-256(identity_b || nonce_b): whatever the deployment binds a proof to, hashed to 32 bytes
static void contexts_for(int n, const std::vector<uint8_t> &nonces, std::vector<uint8_t> &out)
{
    out.resize((size_t)n * 32);
    for (int b = 0; b < n; b++) {
        std::string m = "client-" + std::to_string(b) + "@example.org";
        m.append(reinterpret_cast<const char *>(&nonces[(size_t)b * 16]), 16);
        kosk_host_sha3_256(&out[(size_t)b * 32], reinterpret_cast<const uint8_t *>(m.data()), m.size());
    }
}

int main(int argc, char **argv)
{
    const int k = argc > 1 ? atoi(argv[1]) : 3, n = argc > 2 ? atoi(argv[2]) : 4;
    if (k < 2 || k > 4 || n < 1) { fprintf(stderr, "usage: enrol_bound [2|3|4] [n >= 1]\n"); return 2; }
    const size_t pkb = kosk_pk_bytes(k), skb = kosk_sk_bytes(k), pib = kosk_proof_bytes(k), ctb = kosk_ct_bytes(k);
    kosk_ctx *h = nullptr;
    if (kosk_create(&h, 0, k, n)) { fprintf(stderr, "kosk_create: %s\n", kosk_last_error(nullptr)); return 1; }
    kosk_set_randombytes(h, [](void *, uint8_t *out, size_t len) { fill(out, len); }, nullptr);
    kosk_set_entropy(h, KOSK_ENTROPY_SEED);

    std::vector<uint8_t> pk(n * pkb), sk(n * skb), pi(n * pib), ok(n), ct(n * ctb), ss(n * KOSK_SS_BYTES), ss2(n * KOSK_SS_BYTES), done(n);
    for (int b = 0; b < n; b++) { // 1. keys that exist before any proof is asked for
        uint8_t seed[64];
        fill(seed, sizeof seed);
        MUST(kosk_keygen(k, seed, &pk[b * pkb], &sk[b * skb], nullptr, nullptr, nullptr, nullptr));
    }
    std::vector<uint8_t> nonces((size_t)n * 16), ctx, ctx_replay;
    fill(nonces.data(), nonces.size()); // 2. the registrar's challenges
    contexts_for(n, nonces, ctx);

    MUST(kosk_set_contexts(h, n, ctx.data(), 32)); // 3. the clients' side: armed, every proof is bound to (its pk, its context)
    MUST(kosk_prove_keys_batch(h, n, sk.data(), nullptr, 0, pi.data(), ok.data()));
    for (int b = 0; b < n; b++)
        if (!ok[b]) { printf("[result] enrol_bound FAILED (key %d refused)\n", b); return 1; }

    MUST(kosk_set_contexts(h, n, ctx.data(), 32)); // 4. the registrar's side: armed with the contexts IT issued
    MUST(kosk_verify_batch(h, n, pi.data(), pk.data(), ok.data()));
    MUST(kosk_kem_enc_verified(h, n, nullptr, ct.data(), ss.data(), done.data())); // 5.
    MUST(kosk_kem_dec_batch(h, n, ct.data(), sk.data(), ss2.data()));              // 6.
    int accepted = 0, agree = 0;
    for (int b = 0; b < n; b++) {
        accepted += ok[b] && done[b];
        agree += done[b] && !memcmp(&ss[b * KOSK_SS_BYTES], &ss2[b * KOSK_SS_BYTES], KOSK_SS_BYTES);
    }
    printf("[enrol] kyber_k %d: %d bound proofs, %d accepted, %d shared secrets agree\n", k, n, accepted, agree);

    fill(nonces.data(), nonces.size()); // 7. a replay: the same pairs against the registrar's NEXT challenges
    contexts_for(n, nonces, ctx_replay);
    MUST(kosk_set_contexts(h, n, ctx_replay.data(), 32));
    MUST(kosk_verify_batch(h, n, pi.data(), pk.data(), ok.data()));
    int replayed = 0;
    for (int b = 0; b < n; b++) replayed += ok[b];
    MUST(kosk_set_contexts(h, 0, nullptr, 0)); // and on a verifier that knows nothing of contexts
    MUST(kosk_verify_batch(h, n, pi.data(), pk.data(), ok.data()));
    int unbound = 0;
    for (int b = 0; b < n; b++) unbound += ok[b];
    printf("[enrol] replay under new nonces: %d accepted; on a disarmed handle: %d accepted\n", replayed, unbound);
    kosk_destroy(h);
    if (accepted != n || agree != n || replayed || unbound) { printf("[result] enrol_bound FAILED\n"); return 1; }
    printf("[result] enrol_bound success\n");
    return 0;
}
