// Host build of the witness recovery (csrc/kosk_witness_dev.hpp): the same code k_witness_from_sk runs on gfx950, one "workgroup"
// executed as thread 0 of 1, behind a host decoding of the embedded pk that mirrors launch_decode_pk (t-hat: the 12-bit fields as they
// stand; A[i][j] = XOF(rho, j, i), indcpa.c:168-193).  A stand-alone program: tests/test_keyproof_host.py runs it on files, and it is the
// program for a sanitizer run of this code (every buffer below is a heap block of exactly the size the device buffers have):
//
//   c++ -O2 -std=c++20 -I mpcith_kyber_kosk_amd/csrc tools/witness_host_model.cpp -o witness_host_model
//   c++ -O1 -g -std=c++20 -fsanitize=address,undefined -fno-sanitize-recover=all -I mpcith_kyber_kosk_amd/csrc tools/witness_host_model.cpp -o witness_host_model_san
//
//   witness_host_model K in.bin out.bin
// in.bin : n secret-key records of 768 K + 96 bytes.   out.bin : [n][2 K][256] int16 (s then e) | [n][384 K + 32] copied pk bytes | [n] ok
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kosk_witness_dev.hpp"

using namespace kosk;
using namespace kosk::wit;

namespace {

template <class T> T *block(size_t count) // 16-byte aligned, exactly count elements (rounded up to the alignment only)
{
    void *p = aligned_alloc(16, (count * sizeof(T) + 15) / 16 * 16);
    if (!p) { fprintf(stderr, "out of memory\n"); exit(2); }
    return static_cast<T *>(p);
}

int run(int K, const std::vector<uint8_t> &in, std::vector<uint8_t> &out)
{
    const Dims D = dims(K);
    if (in.empty() || in.size() % (size_t)D.sk) { fprintf(stderr, "input is not a whole number of %d-byte records\n", D.sk); return 2; }
    const size_t n = in.size() / (size_t)D.sk, se_bytes = (size_t)2 * K * 512;
    out.assign(n * (se_bytes + (size_t)D.pk + 1), 0);
    uint8_t *sk = block<uint8_t>((size_t)D.sk), *pk = block<uint8_t>((size_t)D.pk), ok = 0;
    int16_t *A = block<int16_t>((size_t)K * K * 256), *se = block<int16_t>((size_t)2 * K * 256);
    uint16_t *t = block<uint16_t>((size_t)K * 256), *L = block<uint16_t>((size_t)2 * K * 256);
    int rc = 0;
    for (size_t b = 0; b < n && !rc; b++) {
        memcpy(sk, in.data() + b * (size_t)D.sk, (size_t)D.sk);
        const uint8_t *epk = sk + D.pvb;
        for (int c = 0; c < K * 128; c++) { // k_decode_pk
            const uint8_t *a = epk + 3 * c;
            t[2 * c] = (uint16_t)(((uint32_t)a[0] | ((uint32_t)a[1] << 8)) & 0xFFF);
            t[2 * c + 1] = (uint16_t)(((uint32_t)(a[1] >> 4) | ((uint32_t)a[2] << 4)) & 0xFFF);
        }
        uint64_t rho[4];
        memcpy(rho, epk + D.pvb, 32);
        for (int i = 0; i < K && !rc; i++)
            for (int j = 0; j < K; j++)
                if (!matrix_entry(rho, j, i, 32, A + (i * K + j) * 256)) { fprintf(stderr, "gen_matrix block limit\n"); rc = 3; break; }
        if (rc) break;
        const uint32_t bad = recover_block(D, L, 0, 1, sk, A, t);
        store_block(D, L, 0, 1, bad, epk, se, pk, &ok);
        memcpy(out.data() + b * se_bytes, se, se_bytes);
        memcpy(out.data() + n * se_bytes + b * (size_t)D.pk, pk, (size_t)D.pk);
        out[n * (se_bytes + (size_t)D.pk) + b] = ok;
    }
    free(sk); free(pk); free(A); free(se); free(t); free(L);
    return rc;
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 4) { fprintf(stderr, "usage: %s K in.bin out.bin\n", argv[0]); return 2; }
    const int K = atoi(argv[1]);
    if (K < 2 || K > 4) { fprintf(stderr, "K must be 2, 3 or 4\n"); return 2; }
    FILE *f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    std::vector<uint8_t> in, out;
    uint8_t buf[65536];
    for (size_t got; (got = fread(buf, 1, sizeof buf, f)) > 0;) in.insert(in.end(), buf, buf + got);
    fclose(f);
    const int rc = run(K, in, out);
    if (rc) return rc;
    f = fopen(argv[3], "wb");
    if (!f) { perror(argv[3]); return 2; }
    const bool wrote = fwrite(out.data(), 1, out.size(), f) == out.size();
    return (fclose(f) == 0 && wrote) ? 0 : 2;
}
