// The offline bank on the C ABI (include/kosk_mi355x.h): a party that proves keys under a fresh context when the nonce
// arrives, and has done everything that needs no key beforehand:
//   1. while idle: room for 2 n proofs' offline material in HBM, filled in two calls         kosk_bank_reserve, kosk_bank_fill
//   2. the keys arrive: n ordinary key pairs                                                  kosk_kem_keypair_batch
//   3. the nonces arrive: the handle is armed, n proofs cost the online part only             kosk_set_contexts, kosk_prove_keys_banked_batch
//   4. the verifier accepts them under those contexts and not without                         kosk_verify_batch
//   5. an entry is used once: the level went down by n, and a second batch uses the next n
//   6. asking for more than the bank holds is refused and consumes nothing
//   7. kosk_wipe_secrets empties the bank                                                     kosk_wipe_secrets, kosk_bank_level
// One line per stage, ending in "= 1" where it holds.
//   bank_online [kyber_k = 3] [n = 4]
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "kosk_mi355x.h"

static void randombytes(uint8_t *out, size_t outlen)
{
    static std::mt19937_64 rng(20261020); // a deterministic stand-in: this is an example, not a key generator
    for (size_t i = 0; i < outlen; i++) out[i] = (uint8_t)rng();
}

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
    const int n = argc > 2 ? atoi(argv[2]) : 4;
    if (k < 2 || k > 4 || n < 1) { fprintf(stderr, "usage: bank_online [2|3|4] [n >= 1]\n"); return 2; }
    const size_t pkb = kosk_pk_bytes(k), skb = kosk_sk_bytes(k), pib = kosk_proof_bytes(k);
    kosk_ctx *h = nullptr;
    if (kosk_create(&h, 0, k, n)) { fprintf(stderr, "kosk_create: %s\n", kosk_last_error(nullptr)); return 1; }
    kosk_set_randombytes(h, [](void *, uint8_t *out, size_t len) { randombytes(out, len); }, nullptr);
    kosk_set_entropy(h, KOSK_ENTROPY_SEED); // one 32-byte draw per entry and per proof
    std::vector<uint8_t> pk(n * pkb), sk(n * skb), pi(n * pib), pi2(n * pib), proven(n), ok(n), ctx(n * 32);
    int all = 1, ready = -1, cap = -1;
    auto stage = [&](const char *what, bool good) {
        printf("[bank_online] kyber_k %d, %d proofs: %s = %d\n", k, n, what, (int)good);
        all &= (int)good;
    };

    MUST(kosk_bank_reserve(h, 2 * n));
    MUST(kosk_bank_fill(h, n, nullptr, 0, nullptr, 0));
    MUST(kosk_bank_fill(h, n, nullptr, 0, nullptr, 0));
    MUST(kosk_bank_level(h, &ready, &cap));
    stage("kosk_bank_reserve + kosk_bank_fill: the bank is full", ready == 2 * n && cap == 2 * n);

    MUST(kosk_kem_keypair_batch(h, n, nullptr, pk.data(), sk.data()));
    randombytes(ctx.data(), ctx.size());
    MUST(kosk_set_contexts(h, n, ctx.data(), 32));
    MUST(kosk_prove_keys_banked_batch(h, n, sk.data(), nullptr, 0, nullptr, 0, pi.data(), proven.data()));
    MUST(kosk_verify_batch(h, n, pi.data(), pk.data(), ok.data()));
    int good = 0;
    for (int b = 0; b < n; b++) good += proven[b] == 1 && ok[b] == 1;
    stage("kosk_prove_keys_banked_batch + kosk_verify_batch under the contexts: every key proven and verified", good == n);

    MUST(kosk_set_contexts(h, 0, nullptr, 0));
    MUST(kosk_verify_batch(h, n, pi.data(), pk.data(), ok.data()));
    int stray = 0;
    for (int b = 0; b < n; b++) stray += ok[b] != 0;
    stage("the same proofs without the contexts: none accepted", stray == 0);

    MUST(kosk_bank_level(h, &ready, &cap));
    MUST(kosk_prove_keys_banked_batch(h, n, sk.data(), nullptr, 0, nullptr, 0, pi2.data(), proven.data()));
    MUST(kosk_verify_batch(h, n, pi2.data(), pk.data(), ok.data()));
    good = 0;
    for (int b = 0; b < n; b++) good += proven[b] == 1 && ok[b] == 1 && memcmp(&pi[b * pib], &pi2[b * pib], pib) != 0;
    stage("a second batch takes the next entries: level n before it, other proofs, all verified", ready == n && good == n);

    long puts = 0, takes = 0;
    kosk_path_count(h, 25, &puts);
    kosk_path_count(h, 26, &takes);
    stage("launches counted (ids 25, 26)", puts == 2 && takes == 2);

    MUST(kosk_bank_fill(h, 1, nullptr, 0, nullptr, 0));
    std::vector<uint8_t> keep(pi2);
    // (refused on the level alone, before a record or a buffer is touched)
    const int rc = kosk_prove_keys_banked_batch(h, 2, sk.data(), nullptr, 0, nullptr, 0, pi2.data(), proven.data());
    MUST(kosk_bank_level(h, &ready, &cap));
    stage("more proofs than entries: refused, nothing consumed, nothing written", rc == -1 && ready == 1 && keep == pi2);

    MUST(kosk_wipe_secrets(h));
    MUST(kosk_bank_level(h, &ready, &cap));
    const int rc2 = kosk_prove_keys_banked_batch(h, 1, sk.data(), nullptr, 0, nullptr, 0, pi2.data(), proven.data());
    stage("kosk_wipe_secrets: the bank is empty and says so", ready == 0 && rc2 == -1 && strstr(kosk_last_error(h), "bank is empty") != nullptr);
    kosk_destroy(h);
    printf("[result] bank_online success = %d\n", all);
    return all ? 0 : 1;
}
