// The host definition of kosk-regtree-v1 (csrc/kosk_regtree.hpp) as a stand-alone program: tests/test_registry_tree_host.py builds it with
// ASan + UBSan and runs it.  It rebuilds small trees node by node, walks every path up to the root (depths 0, 1, 3), walks one path at depth
// 31 in both directions of every bit, checks the pinned prefixes of E, that the three hashes are separated, unaligned operands, and every
// refusal.  Prints "regtree checks <n> failures 0".
#include <cstdio>
#include <cstring>
#include <vector>

#include "kosk_regtree.hpp"

using namespace kosk;

static int checks = 0, failures = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        checks++;                                                       \
        if (!(x)) { failures++; printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #x); } \
    } while (0)

static void fill(uint8_t *p, size_t n, unsigned seed)
{
    for (size_t i = 0; i < n; i++) p[i] = (uint8_t)(seed = seed * 1103515245u + 12345u, seed >> 16);
}

// the tree over `cap` slots, slot s occupied where occ[s]; every path against the root
static void small_tree(int K, int cap, const std::vector<int> &occ)
{
    const int D = regtree::depth(cap), P = 1 << D;
    std::vector<std::vector<uint8_t>> lv((size_t)D + 1);
    std::vector<uint8_t> h((size_t)cap * 32);
    fill(h.data(), h.size(), 77u + (unsigned)cap);
    lv[0].resize((size_t)P * 32);
    for (int s = 0; s < P; s++) CHECK(regtree::leaf(K, s < cap && occ[(size_t)s] ? &h[(size_t)s * 32] : nullptr, &lv[0][(size_t)s * 32]) == 0);
    for (int l = 1; l <= D; l++) {
        lv[(size_t)l].resize((size_t)(P >> l) * 32);
        for (int i = 0; i < (P >> l); i++)
            CHECK(regtree::node(&lv[(size_t)l - 1][(size_t)(2 * i) * 32], &lv[(size_t)l - 1][(size_t)(2 * i + 1) * 32], &lv[(size_t)l][(size_t)i * 32]) == 0);
    }
    const uint8_t *root = lv[(size_t)D].data();
    for (int s = 0; s < P; s++) {
        std::vector<uint8_t> path((size_t)D * 32 + 1), got(32);
        for (int l = 0; l < D; l++) memcpy(&path[(size_t)l * 32], &lv[(size_t)l][(size_t)((s >> l) ^ 1) * 32], 32);
        const bool full = s < cap && occ[(size_t)s];
        CHECK(regtree::root_from_path(K, D, s, full ? &h[(size_t)s * 32] : nullptr, D ? path.data() : nullptr, got.data()) == 0);
        CHECK(!memcmp(got.data(), root, 32));
        // the wrong claim about the slot gives another root
        uint8_t other[32];
        fill(other, 32, 5u + (unsigned)s);
        CHECK(regtree::root_from_path(K, D, s, full ? nullptr : other, D ? path.data() : nullptr, got.data()) == 0);
        CHECK(memcmp(got.data(), root, 32) != 0);
        if (D) {
            path[(size_t)(s % D) * 32 + 7] ^= 0x10;
            CHECK(regtree::root_from_path(K, D, s, full ? &h[(size_t)s * 32] : nullptr, path.data(), got.data()) == 0);
            CHECK(memcmp(got.data(), root, 32) != 0);
        }
    }
}

int main()
{
    CHECK(regtree::depth(1) == 0 && regtree::depth(2) == 1 && regtree::depth(3) == 2 && regtree::depth(4) == 2 && regtree::depth(5) == 3);
    CHECK(regtree::depth(1024) == 10 && regtree::depth(1025) == 11 && regtree::depth(1 << 20) == 20 && regtree::depth((1 << 20) + 1) == 21);
    CHECK(regtree::depth(0) == -1 && regtree::depth(-1) == -1 && regtree::depth(2147483647) == 31);
    CHECK(regtree::tree_bytes(1) == 32 && regtree::tree_bytes(3) == 7 * 32 && regtree::tree_bytes(1025) == 4095 * 32 && regtree::tree_bytes(0) == 0 && regtree::tree_bytes(-7) == 0);
    CHECK(regtree::level_offset(3, 0) == 0 && regtree::level_offset(3, 1) == 8 * 32 && regtree::level_offset(3, 3) == 14 * 32 && regtree::level_offset(0, 0) == 0);
    CHECK(regtree::tiers(0) == 1 && regtree::tiers(10) == 1 && regtree::tiers(11) == 2 && regtree::tiers(20) == 2 && regtree::tiers(21) == 3);
    CHECK(regtree::subtrees(0) == 1 && regtree::subtrees(10) == 1 && regtree::subtrees(11) == 2 && regtree::subtrees(20) == 1024);

    // E begins 2aca555f / dd6d2c3c / a93686a2 for kyber_k 2 / 3 / 4
    const uint8_t want[3][4] = {{0x2a, 0xca, 0x55, 0x5f}, {0xdd, 0x6d, 0x2c, 0x3c}, {0xa9, 0x36, 0x86, 0xa2}};
    for (int K = 2; K <= 4; K++) {
        uint8_t e[32];
        CHECK(regtree::leaf(K, nullptr, e) == 0 && !memcmp(e, want[K - 2], 4));
    }
    // the three kinds are separated, and K enters both leaves
    {
        uint8_t z[64] = {0}, a[32], b[32], c[32], d[32];
        CHECK(regtree::leaf(2, z, a) == 0 && regtree::leaf(3, z, b) == 0 && regtree::leaf(2, nullptr, c) == 0 && regtree::node(z, z + 32, d) == 0);
        CHECK(memcmp(a, b, 32) && memcmp(a, c, 32) && memcmp(a, d, 32) && memcmp(c, d, 32));
        // node is not symmetric
        uint8_t x[32], y[32], xy[32], yx[32];
        fill(x, 32, 1); fill(y, 32, 2);
        CHECK(regtree::node(x, y, xy) == 0 && regtree::node(y, x, yx) == 0 && memcmp(xy, yx, 32));
        // operands at odd addresses, the result over an operand
        std::vector<uint8_t> odd(1 + 32 + 32 + 32);
        memcpy(&odd[1], x, 32); memcpy(&odd[33], y, 32);
        CHECK(regtree::node(&odd[1], &odd[33], &odd[65]) == 0 && !memcmp(&odd[65], xy, 32));
        CHECK(regtree::node(&odd[1], &odd[33], &odd[1]) == 0 && !memcmp(&odd[1], xy, 32));
    }

    small_tree(2, 1, {0});
    small_tree(2, 1, {1});
    small_tree(3, 2, {1, 0});
    small_tree(4, 3, {0, 1, 1});
    small_tree(2, 5, {1, 0, 0, 1, 1});
    small_tree(2, 8, {1, 1, 1, 1, 1, 1, 1, 1});

    // depth 31: the walk by hand against root_from_path, at the lowest, the highest and a mixed slot
    {
        std::vector<uint8_t> path(31 * 32), h(32);
        fill(path.data(), path.size(), 9);
        fill(h.data(), 32, 10);
        const int32_t slots[3] = {0, 2147483647, 0x2aaaaaaa};
        for (int32_t s : slots) {
            uint8_t cur[32], got[32];
            CHECK(regtree::leaf(3, h.data(), cur) == 0);
            for (int l = 0; l < 31; l++) {
                if ((s >> l) & 1) CHECK(regtree::node(&path[(size_t)l * 32], cur, cur) == 0);
                else CHECK(regtree::node(cur, &path[(size_t)l * 32], cur) == 0);
            }
            CHECK(regtree::root_from_path(3, 31, s, h.data(), path.data(), got) == 0 && !memcmp(got, cur, 32));
        }
    }

    // refusals
    {
        uint8_t a[32] = {0}, out[32], path[64] = {0};
        CHECK(regtree::leaf(1, a, out) == -1 && regtree::leaf(5, nullptr, out) == -1 && regtree::leaf(2, a, nullptr) == -1);
        CHECK(regtree::node(nullptr, a, out) == -1 && regtree::node(a, nullptr, out) == -1 && regtree::node(a, a, nullptr) == -1);
        CHECK(regtree::root_from_path(1, 1, 0, a, path, out) == -1 && regtree::root_from_path(5, 1, 0, a, path, out) == -1);
        CHECK(regtree::root_from_path(2, -1, 0, a, path, out) == -1 && regtree::root_from_path(2, 32, 0, a, path, out) == -1);
        CHECK(regtree::root_from_path(2, 1, -1, a, path, out) == -1 && regtree::root_from_path(2, 1, 2, a, path, out) == -1);
        CHECK(regtree::root_from_path(2, 0, 1, a, nullptr, out) == -1 && regtree::root_from_path(2, 0, 0, a, nullptr, out) == 0);
        CHECK(regtree::root_from_path(2, 1, 0, a, nullptr, out) == -1 && regtree::root_from_path(2, 1, 0, a, path, nullptr) == -1);
        CHECK(regtree::root_from_path(2, 2, 3, nullptr, path, out) == 0);
    }
    printf("regtree checks %d failures %d\n", checks, failures);
    return failures ? 1 : 0;
}
