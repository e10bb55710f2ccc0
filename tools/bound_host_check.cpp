// Stand-alone check of the host Fiat-Shamir functions with a binding value (kosk-bind-v1, csrc/kosk_host.cpp): the batch forms, whose
// multi-buffer hash takes B as a suffix of the last block, against the plain sponge on a copy `table || B`, at whatever SIMD width the
// environment selects (KOSK_FS_WIDTH = 8 / 4 / 1, KOSK_HOST_SCALAR), with a ragged batch and a table stride that is not the table size.
//   c++ -std=c++20 -O1 -g -fsanitize=address,undefined -I mpcith_kyber_kosk_amd/csrc tools/bound_host_check.cpp mpcith_kyber_kosk_amd/csrc/kosk_host.cpp -lpthread
// (tests/test_bound_host.py builds and runs it that way)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kosk_host.hpp"
using namespace kosk;

int main()
{
    int bad = 0;
    for (int K = 2; K <= 4; K++) {
        Params P;
        make_params(K, P);
        const int n = 13; // ragged for the widths 4 and 8
        const size_t T = (size_t)NPARTY * 32, stride = T + 8;
        std::vector<uint8_t> tabs(n * stride), bind((size_t)n * 32);
        srand(1000 + K);
        for (auto &x : tabs) x = (uint8_t)rand();
        for (auto &x : bind) x = (uint8_t)rand();
        std::vector<uint16_t> alpha((size_t)n * 80), I((size_t)n * 1312), rest((size_t)n * 1312);
        fs_alpha_batch(P, n, tabs.data(), stride, alpha.data(), 80, 4, nullptr, nullptr, bind.data());
        fs_opened_batch(n, tabs.data(), stride, I.data(), rest.data(), 1312, 4, nullptr, true, nullptr, bind.data());
        for (int b = 0; b < n; b++) {
            std::vector<uint8_t> m(T + 32);
            memcpy(m.data(), &tabs[b * stride], T);
            memcpy(m.data() + T, &bind[(size_t)b * 32], 32);
            uint8_t h[32], a_[2 * 80];
            sha3_256(h, m.data(), m.size());
            shake256_prf(a_, (size_t)2 * P.J, h, 1);
            for (int i = 0; i < P.J; i++) bad += alpha[(size_t)b * 80 + i] != (uint16_t)(((a_[2 * i] << 8) | a_[2 * i + 1]) % Q);
            uint16_t a1[80], I1[NOPEN], r1[NREST];
            fs_alpha(P, &tabs[b * stride], a1, &bind[(size_t)b * 32]); // the single-proof forms agree with the batch forms
            bad += memcmp(a1, &alpha[(size_t)b * 80], (size_t)2 * P.J) != 0;
            fs_opened(&tabs[b * stride], I1, r1, &bind[(size_t)b * 32]);
            bad += memcmp(I1, &I[(size_t)b * 1312], 2 * NOPEN) != 0 || memcmp(r1, &rest[(size_t)b * 1312], 2 * NREST) != 0;
            uint16_t a2[80]; // and without a binding value the transcript is the reference's
            fs_alpha(P, &tabs[b * stride], a2);
            sha3_256(h, &tabs[b * stride], T);
            shake256_prf(a_, (size_t)2 * P.J, h, 1);
            for (int i = 0; i < P.J; i++) bad += a2[i] != (uint16_t)(((a_[2 * i] << 8) | a_[2 * i + 1]) % Q);
        }
        uint8_t pk[1568], ctx[32], B[32], m[84] = {'k', 'o', 's', 'k', '-', 'b', 'i', 'n', 'd', '-', 'v', '1', 0, 0, 0, 0, (uint8_t)K};
        for (auto &x : pk) x = (uint8_t)rand();
        for (auto &x : ctx) x = (uint8_t)rand();
        bind_value(P, pk, ctx, B);
        sha3_256(m + 20, pk, P.pk_bytes);
        memcpy(m + 52, ctx, 32);
        uint8_t want[32];
        sha3_256(want, m, sizeof m);
        bad += memcmp(B, want, 32) != 0;
    }
    printf("bound_host_check: simd width %d, mismatches %d\n", sha3_multi_width(), bad);
    return bad != 0;
}
