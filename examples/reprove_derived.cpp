// One key, two enrolments, no entropy source and no stored seed (format kosk-keyseed-v1) on the C ABI:
//   1. the holder has nothing but a Kyber key pair                            kosk_keygen (host; any Kyber implementation's key does)
//   2. a registrar sends nonce A; context_A = SHA3-256(identity || nonce_A)   kosk_set_contexts + kosk_prove_keys_derived_batch
//   3. later it sends nonce B: another context, another (independent) tape    the same two calls
//   4. each proof verifies under its own context and not under the other      kosk_verify_batch
//   5. nonce A again gives the bytes of step 2: the call is a pure function of (sk, K, context)
//   reprove_derived [kyber_k = 3]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "kosk_mi355x.h"

#define MUST(x)                                                                       \
    do {                                                                              \
        if (x) {                                                                      \
            fprintf(stderr, "%s: %s\n", #x, kosk_last_error(h));                      \
            return 1;                                                                 \
        }                                                                             \
    } while (0)

static void context_for(const char *nonce, uint8_t out[32])
{
    const std::string m = std::string("device-0017@example.org") + nonce;
    kosk_host_sha3_256(out, reinterpret_cast<const uint8_t *>(m.data()), m.size());
}

int main(int argc, char **argv)
{
    const int k = argc > 1 ? atoi(argv[1]) : 3;
    if (k < 2 || k > 4) { fprintf(stderr, "usage: reprove_derived [2|3|4]\n"); return 2; }
    const size_t pkb = kosk_pk_bytes(k), skb = kosk_sk_bytes(k), pib = kosk_proof_bytes(k);
    kosk_ctx *h = nullptr;
    if (kosk_create(&h, 0, k, 1)) { fprintf(stderr, "kosk_create: %s\n", kosk_last_error(nullptr)); return 1; }

    std::vector<uint8_t> pk(pkb), sk(skb), piA(pib), piB(pib), piA2(pib);
    uint8_t keyseed[64], ctxA[32], ctxB[32], ok = 0;
    for (int i = 0; i < 64; i++) keyseed[i] = (uint8_t)(7 * i + 1); // the key exists before anything else: a fixed stand-in
    MUST(kosk_keygen(k, keyseed, pk.data(), sk.data(), nullptr, nullptr, nullptr, nullptr));
    context_for("nonce-A", ctxA);
    context_for("nonce-B", ctxB);

    auto prove = [&](const uint8_t *ctx, std::vector<uint8_t> &pi) { // nothing goes in but the key and the context
        if (kosk_set_contexts(h, 1, ctx, 32)) return 1;
        if (kosk_prove_keys_derived_batch(h, 1, sk.data(), nullptr, 0, pi.data(), &ok)) return 1;
        return ok ? 0 : 1;
    };
    auto verify = [&](const uint8_t *ctx, const std::vector<uint8_t> &pi, int &accepted) {
        uint8_t v = 0;
        if (kosk_set_contexts(h, 1, ctx, 32) || kosk_verify_batch(h, 1, pi.data(), pk.data(), &v)) return 1;
        accepted = v;
        return 0;
    };
    MUST(prove(ctxA, piA));
    MUST(prove(ctxB, piB));
    MUST(prove(ctxA, piA2));
    int aa = 0, bb = 0, ab = 0, ba = 0;
    MUST(verify(ctxA, piA, aa));
    MUST(verify(ctxB, piB, bb));
    MUST(verify(ctxB, piA, ab));
    MUST(verify(ctxA, piB, ba));
    kosk_destroy(h);

    printf("[reprove] kyber_k %d: proof A verifies under context A = %d\n", k, aa);
    printf("[reprove] proof B verifies under context B = %d\n", bb);
    printf("[reprove] proof A is refused under context B = %d\n", !ab);
    printf("[reprove] proof B is refused under context A = %d\n", !ba);
    printf("[reprove] the two proofs differ = %d\n", memcmp(piA.data(), piB.data(), pib) != 0);
    printf("[reprove] nonce A again gives the same bytes = %d\n", memcmp(piA.data(), piA2.data(), pib) == 0);
    const int all = aa && bb && !ab && !ba && memcmp(piA.data(), piB.data(), pib) != 0 && memcmp(piA.data(), piA2.data(), pib) == 0;
    printf("[result] reprove_derived success = %d\n", all);
    return all ? 0 : 1;
}
