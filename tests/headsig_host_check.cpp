// The host definition of kosk-headsig-v1 (csrc/kosk_headsig.hpp) as a stand-alone program: tests/test_headsig_host.py builds it with
// ASan + UBSan and runs it.  It builds the trees of heights 1 and 2 node by node (written here, on the header's sponge states), checks the
// root against public_from_seed, signs every leaf's head the way the format text says and checks that verify accepts it from buffers at
// misalignments 1, 2, 5 and 7 and rejects every flipped field, a wrong size, a wrong kyber_k and an advanced chain; then the statement's
// bytes and every refusal.  Prints "headsig checks <n> failures 0".
#include <array>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kosk_headsig.hpp"

using namespace kosk;

static int checks = 0, failures = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        checks++;                                                       \
        if (!(x)) { failures++; printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #x); } \
    } while (0)

typedef std::array<uint64_t, 4> Hash;

static void fill(uint8_t *p, size_t n, unsigned seed)
{
    for (size_t i = 0; i < n; i++) p[i] = (uint8_t)(seed = seed * 1103515245u + 12345u, seed >> 16);
}

struct Tree {
    int h;
    headsig::Id id;
    uint64_t seed[4];
    std::vector<Hash> T; // T[r], r = 1 .. 2^(h+1) - 1
    Tree(int h_, const uint8_t *seed_, const uint8_t *idp) : h(h_), T((size_t)2 << h_)
    {
        headsig::id_in(id, idp);
        memcpy(seed, seed_, 32);
        for (uint32_t q = 0; q < (1u << h); q++) {
            uint64_t y[headsig::Y_WORDS];
            for (int i = 0; i < headsig::CHAINS; i++) {
                uint64_t t[4];
                headsig::secret_start(id, q, (uint32_t)i, seed, t);
                headsig::chain_run(id, q, (uint32_t)i, 0, headsig::STEPS, t);
                memcpy(y + 4 * i, t, 32);
            }
            uint64_t leaf[4];
            headsig::leaf_from_ends(id, h, q, y, leaf);
            memcpy(T[(1u << h) + q].data(), leaf, 32);
        }
        for (uint32_t r = (1u << h) - 1; r >= 1; r--) {
            uint64_t s[25], l[4], rr[4], o[4];
            memcpy(l, T[2 * r].data(), 32);
            memcpy(rr, T[2 * r + 1].data(), 32);
            headsig::node_state(s, id, r, l, rr);
            headsig::finish(s, o);
            memcpy(T[r].data(), o, 32);
        }
    }
    std::vector<uint8_t> sign(int K, const uint8_t *root, uint32_t q) const
    {
        std::vector<uint8_t> sig(headsig::sig_bytes(h));
        headsig::le32_out(sig.data(), (uint32_t)h);
        headsig::le32_out(sig.data() + 4, q);
        uint64_t c[4], r[4], Q[4], s[25];
        headsig::secret_start(id, q, headsig::TAG_C, seed, c);
        memcpy(sig.data() + headsig::SIG_C, c, 32);
        memcpy(r, root, 32);
        headsig::digest_state(s, id, q, c, r, q, K);
        headsig::finish(s, Q);
        for (int i = 0; i < headsig::CHAINS; i++) {
            uint64_t t[4];
            headsig::secret_start(id, q, (uint32_t)i, seed, t);
            headsig::chain_run(id, q, (uint32_t)i, 0, (int)headsig::coefficient(Q, i), t);
            memcpy(sig.data() + headsig::SIG_Z + 32 * i, t, 32);
        }
        for (int l = 0; l < h; l++) memcpy(sig.data() + headsig::SIG_PATH + 32 * l, T[(((1u << h) + q) >> l) ^ 1].data(), 32);
        return sig;
    }
};

// verify from copies that start `off` bytes into their allocations
static int verify_at(int off, const uint8_t *pub, int K, const uint8_t *root, int size, const std::vector<uint8_t> &sig)
{
    std::vector<uint8_t> p(headsig::PUB_BYTES + off), r(32 + off), g(sig.size() + off);
    memcpy(p.data() + off, pub, headsig::PUB_BYTES);
    memcpy(r.data() + off, root, 32);
    memcpy(g.data() + off, sig.data(), sig.size());
    return headsig::verify(p.data() + off, K, r.data() + off, size, g.data() + off);
}

int main()
{
    uint8_t seed[32], id[16], root[32];
    fill(seed, 32, 1);
    fill(id, 16, 2);
    CHECK(headsig::sig_bytes(0) == 0 && headsig::sig_bytes(25) == 0 && headsig::sig_bytes(-1) == 0 && headsig::sig_bytes(1) == 1168 && headsig::sig_bytes(24) == 1904);
    for (int h = 1; h <= 2; h++) {
        const Tree tree(h, seed, id);
        std::vector<uint8_t> pubbuf(headsig::PUB_BYTES + 3);
        uint8_t *pub = pubbuf.data() + 3; // unaligned
        CHECK(headsig::public_from_seed(h, seed, id, pub) == 0);
        CHECK(headsig::le32_in(pub) == (uint32_t)h && !memcmp(pub + headsig::PUB_I, id, 16) && !memcmp(pub + headsig::PUB_ROOT, tree.T[1].data(), 32));
        for (uint32_t q = 0; q < (1u << h); q++) {
            fill(root, 32, 100 + 8 * h + q);
            const int K = 2 + (int)(q % 3);
            const std::vector<uint8_t> sig = tree.sign(K, root, q);
            for (int off : {0, 1, 2, 5, 7}) CHECK(verify_at(off, pub, K, root, (int)q, sig) == 1);
            CHECK(headsig::verify(pub, K == 4 ? 2 : K + 1, root, (int)q, sig.data()) == 0);
            CHECK(verify_at(1, pub, K, root, (int)(q ^ 1), sig) == 0);
            for (size_t at = 0; q + 1 == (1u << h) && at < sig.size(); at += (at < 16 ? 1 : 23)) { // the last leaf: every header byte, then a byte of C and of every 32-byte field
                std::vector<uint8_t> bad = sig;
                bad[at] ^= (uint8_t)(1u << (at % 8));
                CHECK(verify_at((int)(at % 8), pub, K, root, (int)q, bad) == 0);
            }
            for (int at = 0; at < 32; at += 5) {
                uint8_t r2[32];
                memcpy(r2, root, 32);
                r2[at] ^= 0x80;
                CHECK(headsig::verify(pub, K, r2, (int)q, sig.data()) == 0);
            }
            for (int at = 4; at < (int)headsig::PUB_BYTES; at += 7) {
                uint8_t p2[headsig::PUB_BYTES];
                memcpy(p2, pub, sizeof p2);
                p2[at] ^= 1;
                CHECK(headsig::verify(p2, K, root, (int)q, sig.data()) == 0);
            }
            // the forgery direction: chain 3 one step further, the checksum chains as they are
            uint64_t c[4], r[4], Q[4], s[25], t[4];
            memcpy(c, sig.data() + headsig::SIG_C, 32);
            memcpy(r, root, 32);
            headsig::digest_state(s, tree.id, q, c, r, q, K);
            headsig::finish(s, Q);
            const int a3 = (int)headsig::coefficient(Q, 3);
            if (a3 < headsig::STEPS) {
                std::vector<uint8_t> forged = sig;
                memcpy(t, sig.data() + headsig::SIG_Z + 32 * 3, 32);
                headsig::chain_run(tree.id, q, 3, a3, a3 + 1, t);
                memcpy(forged.data() + headsig::SIG_Z + 32 * 3, t, 32);
                CHECK(headsig::verify(pub, K, root, (int)q, forged.data()) == 0);
            }
            uint32_t sum = 0;
            for (int i = 0; i < 32; i++) sum += 255 - headsig::coefficient(Q, i);
            CHECK(headsig::coefficient(Q, 32) == (sum >> 8) && headsig::coefficient(Q, 33) == (sum & 255));
        }
        // q = 2^h, as the sole defect of an otherwise well-formed record
        fill(root, 32, 7);
        std::vector<uint8_t> over = tree.sign(3, root, 0);
        headsig::le32_out(over.data() + 4, 1u << h);
        CHECK(headsig::verify(pub, 3, root, 1 << h, over.data()) == 0);
    }
    // the statement, out of and into unaligned buffers, and in place over its own root
    {
        uint8_t buf[64 + 5], want[56];
        fill(root, 32, 9);
        memcpy(want, "kosk-sighead-v1", 16);
        memcpy(want + 16, root, 32);
        headsig::le32_out(want + 48, 0x01020304u);
        headsig::le32_out(want + 52, 4);
        CHECK(headsig::statement(4, root, 0x01020304, buf + 5) == 0 && !memcmp(buf + 5, want, 56));
        memcpy(buf + 1 + 16, root, 32);
        CHECK(headsig::statement(4, buf + 1 + 16, 0x01020304, buf + 1) == 0 && !memcmp(buf + 1, want, 56));
    }
    // refusals
    {
        uint8_t pub[headsig::PUB_BYTES] = {0}, out[56], sig[1168] = {0};
        pub[0] = 1;
        CHECK(headsig::verify(nullptr, 3, root, 0, sig) == -1 && headsig::verify(pub, 3, nullptr, 0, sig) == -1 && headsig::verify(pub, 3, root, 0, nullptr) == -1);
        CHECK(headsig::verify(pub, 1, root, 0, sig) == -1 && headsig::verify(pub, 5, root, 0, sig) == -1 && headsig::verify(pub, 3, root, -1, sig) == -1);
        pub[0] = 0;
        CHECK(headsig::verify(pub, 3, root, 0, sig) == -1);
        pub[0] = 25;
        CHECK(headsig::verify(pub, 3, root, 0, sig) == -1);
        pub[0] = 1;
        CHECK(headsig::verify(pub, 3, root, 0, sig) == 0); // a header of zeros: h differs
        CHECK(headsig::statement(1, root, 0, out) == -1 && headsig::statement(3, nullptr, 0, out) == -1 && headsig::statement(3, root, -1, out) == -1 &&
              headsig::statement(3, root, 0, nullptr) == -1);
        CHECK(headsig::public_from_seed(0, seed, id, pub) == -1 && headsig::public_from_seed(25, seed, id, pub) == -1 &&
              headsig::public_from_seed(1, nullptr, id, pub) == -1 && headsig::public_from_seed(1, seed, nullptr, pub) == -1 &&
              headsig::public_from_seed(1, seed, id, nullptr) == -1);
    }
    printf("headsig checks %d failures %d\n", checks, failures);
    return failures ? 1 : 0;
}
