// The host definition of kosk-regsort-v1 (csrc/kosk_regsort.hpp) as a stand-alone program: tests/test_registry_sorted_host.py builds it with
// ASan + UBSan and runs it.  It sorts small registries on the host, rebuilds their trees node by node, forms the proof record of every query
// (00^32, FF^32, every key and every key +- 1) by the rule of INTEGRATION.md 8.6, and takes each through check_proof: the right kind, and
// NEITHER after a flipped bit in every field; a path at depth 31; unaligned operands; every refusal.  Prints "regsort checks <n> failures 0".
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <utility>
#include <vector>

#include "kosk_regsort.hpp"

using namespace kosk;
typedef std::vector<uint8_t> Bytes;

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
static void le32_out(uint8_t *p, int32_t v)
{
    for (int i = 0; i < 4; i++) p[i] = (uint8_t)((uint32_t)v >> (8 * i));
}
// x +- 1 as a 32-byte big-endian number; false where it does not exist
static bool step(Bytes &x, int dir)
{
    for (int i = 31; i >= 0; i--) {
        if (dir > 0 ? ++x[(size_t)i] != 0 : x[(size_t)i]-- != 0) return true;
    }
    return false;
}

struct Tree {
    int K, D, P;
    std::vector<std::pair<Bytes, int32_t>> ent; // (h, slot), ascending
    std::vector<Bytes> lv;
    const uint8_t *root() const { return lv[(size_t)D].data(); }
    void path(int pos, uint8_t *out) const
    {
        for (int l = 0; l < D; l++) memcpy(out + (size_t)l * 32, &lv[(size_t)l][(size_t)((pos >> l) ^ 1) * 32], 32);
    }
};

static Tree build(int K, int cap, const std::vector<Bytes> &h, const std::vector<int> &occ)
{
    Tree t;
    t.K = K; t.D = regtree::depth(cap); t.P = 1 << t.D;
    for (int s = 0; s < cap; s++)
        if (occ[(size_t)s]) t.ent.push_back({h[(size_t)s], s});
    std::sort(t.ent.begin(), t.ent.end());
    t.lv.resize((size_t)t.D + 1);
    t.lv[0].resize((size_t)t.P * 32);
    for (int i = 0; i < t.P; i++) {
        const bool key = i < (int)t.ent.size();
        CHECK(regsort::leaf(K, key ? t.ent[(size_t)i].first.data() : nullptr, key ? t.ent[(size_t)i].second : 0, &t.lv[0][(size_t)i * 32]) == 0);
    }
    for (int l = 1; l <= t.D; l++) {
        t.lv[(size_t)l].resize((size_t)(t.P >> l) * 32);
        for (int i = 0; i < (t.P >> l); i++)
            CHECK(regsort::node(&t.lv[(size_t)l - 1][(size_t)(2 * i) * 32], &t.lv[(size_t)l - 1][(size_t)(2 * i + 1) * 32], &t.lv[(size_t)l][(size_t)i * 32]) == 0);
    }
    return t;
}

// the record of INTEGRATION.md 8.6 for query x; returns the kind
static int prove(const Tree &t, const Bytes &x, Bytes &rec)
{
    const int m = (int)t.ent.size();
    int lb = 0;
    while (lb < m && t.ent[(size_t)lb].first < x) lb++;
    const bool present = lb < m && t.ent[(size_t)lb].first == x;
    rec.assign(regsort::proof_bytes(t.D), 0);
    const bool left = present || lb >= 1, right = !present && lb < t.P, key = right && lb < m;
    const int pos_l = present ? lb : lb - 1;
    le32_out(&rec[regsort::REC_POS_L], left ? pos_l : -1);
    le32_out(&rec[regsort::REC_FLAGS], (left ? 1 : 0) | (right ? 2 : 0) | (key ? 4 : 0) | (present ? 8 : 0));
    if (left) {
        le32_out(&rec[regsort::REC_SLOT_L], t.ent[(size_t)pos_l].second);
        memcpy(&rec[regsort::REC_H_L], t.ent[(size_t)pos_l].first.data(), 32);
        t.path(pos_l, &rec[regsort::REC_PATHS]);
    }
    if (key) {
        le32_out(&rec[regsort::REC_SLOT_R], t.ent[(size_t)lb].second);
        memcpy(&rec[regsort::REC_H_R], t.ent[(size_t)lb].first.data(), 32);
    }
    if (right) t.path(lb, &rec[regsort::REC_PATHS + (size_t)t.D * 32]);
    return present ? regsort::KIND_PRESENT : regsort::KIND_ABSENT;
}

static void query(const Tree &t, const Bytes &x)
{
    Bytes rec;
    const int kind = prove(t, x, rec);
    CHECK(regsort::check_proof(t.K, t.D, x.data(), rec.data(), t.root()) == kind);
    // a record copied to an odd address reads the same
    Bytes odd(rec.size() + 1 + 32 + 32);
    memcpy(&odd[1], rec.data(), rec.size());
    memcpy(&odd[1 + rec.size()], x.data(), 32);
    memcpy(&odd[1 + rec.size() + 32], t.root(), 32);
    CHECK(regsort::check_proof(t.K, t.D, &odd[1 + rec.size()], &odd[1], &odd[1 + rec.size() + 32]) == kind);
    // the wrong k, the wrong root
    CHECK(regsort::check_proof(t.K == 4 ? 2 : t.K + 1, t.D, x.data(), rec.data(), t.root()) == regsort::KIND_NEITHER);
    Bytes other(t.root(), t.root() + 32);
    other[5] ^= 1;
    CHECK(regsort::check_proof(t.K, t.D, x.data(), rec.data(), other.data()) == regsort::KIND_NEITHER);
    // one flipped bit in every field the verdict rests on
    const uint32_t flags = (uint32_t)regsort::le32_in(&rec[regsort::REC_FLAGS]);
    const bool left = flags & 1, right = flags & 2, key = flags & 4;
    std::vector<size_t> at = {regsort::REC_POS_L, regsort::REC_FLAGS + 1, regsort::REC_FLAGS + 3};
    if (left) { at.push_back(regsort::REC_SLOT_L); at.push_back(regsort::REC_H_L + 31); }
    if (key) { at.push_back(regsort::REC_SLOT_R + 1); at.push_back(regsort::REC_H_R + 31); }
    for (int l = 0; l < t.D; l++) {
        if (left) at.push_back(regsort::REC_PATHS + (size_t)l * 32 + 3);
        if (right) at.push_back(regsort::REC_PATHS + (size_t)(t.D + l) * 32 + 30);
    }
    for (size_t a : at) {
        Bytes bad = rec;
        bad[a] ^= 0x04;
        CHECK(regsort::check_proof(t.K, t.D, x.data(), bad.data(), t.root()) == regsort::KIND_NEITHER);
    }
}

static void registry(int K, int cap, const std::vector<int> &occ, const std::vector<int> &same_as = {})
{
    std::vector<Bytes> h((size_t)cap, Bytes(32));
    for (int s = 0; s < cap; s++) fill(h[(size_t)s].data(), 32, 1000u * (unsigned)cap + (unsigned)s);
    for (size_t s = 0; s < same_as.size(); s++)
        if (same_as[s] >= 0) h[s] = h[(size_t)same_as[s]];
    const Tree t = build(K, cap, h, occ);
    query(t, Bytes(32, 0x00));
    query(t, Bytes(32, 0xFF));
    for (int s = 0; s < cap; s++) {
        if (!occ[(size_t)s]) continue;
        query(t, h[(size_t)s]);
        for (int dir = -1; dir <= 1; dir += 2) {
            Bytes x = h[(size_t)s];
            if (step(x, dir)) query(t, x);
        }
    }
    // PRESENT names the lowest slot of a duplicated key
    for (size_t s = 0; s < same_as.size(); s++) {
        if (same_as[s] < 0 || !occ[s] || !occ[(size_t)same_as[s]]) continue;
        Bytes rec;
        CHECK(prove(t, h[s], rec) == regsort::KIND_PRESENT && regsort::le32_in(&rec[regsort::REC_SLOT_L]) <= same_as[s]);
    }
}

int main()
{
    CHECK(regsort::proof_bytes(0) == 80 && regsort::proof_bytes(1) == 144 && regsort::proof_bytes(20) == 1360 && regsort::proof_bytes(31) == 2064);
    CHECK(regsort::proof_bytes(-1) == 0 && regsort::proof_bytes(32) == 0);

    // Z begins becb0cab / 4681eaa2 / d8d33b6a for kyber_k 2 / 3 / 4, S(00^32, 0) for k = 3 begins 0f9fbb3c
    const uint8_t want[3][4] = {{0xbe, 0xcb, 0x0c, 0xab}, {0x46, 0x81, 0xea, 0xa2}, {0xd8, 0xd3, 0x3b, 0x6a}};
    for (int K = 2; K <= 4; K++) {
        uint8_t z[32];
        CHECK(regsort::leaf(K, nullptr, 0, z) == 0 && !memcmp(z, want[K - 2], 4));
    }
    {
        const uint8_t s0[4] = {0x0f, 0x9f, 0xbb, 0x3c};
        uint8_t zero[64] = {0}, a[32], b[32], c[32], d[32], e[32], f[32];
        CHECK(regsort::leaf(3, zero, 0, a) == 0 && !memcmp(a, s0, 4));
        // the slot, k and the kind enter; the two trees' hashes differ
        CHECK(regsort::leaf(3, zero, 1, b) == 0 && regsort::leaf(2, zero, 0, c) == 0 && regsort::node(zero, zero + 32, d) == 0);
        CHECK(regtree::leaf(3, zero, e) == 0 && regtree::node(zero, zero + 32, f) == 0);
        CHECK(memcmp(a, b, 32) && memcmp(a, c, 32) && memcmp(a, d, 32) && memcmp(a, e, 32) && memcmp(d, f, 32));
        uint8_t x[32], y[32], xy[32], yx[32];
        fill(x, 32, 1); fill(y, 32, 2);
        CHECK(regsort::node(x, y, xy) == 0 && regsort::node(y, x, yx) == 0 && memcmp(xy, yx, 32));
        Bytes odd(1 + 32 + 32 + 32);
        memcpy(&odd[1], x, 32); memcpy(&odd[33], y, 32);
        CHECK(regsort::node(&odd[1], &odd[33], &odd[65]) == 0 && !memcmp(&odd[65], xy, 32));
        CHECK(regsort::leaf(4, &odd[1], 7, &odd[1]) == 0 && regsort::leaf(4, x, 7, a) == 0 && !memcmp(&odd[1], a, 32));
    }

    registry(2, 1, {0});
    registry(2, 1, {1});
    registry(3, 2, {1, 0});
    registry(3, 2, {1, 1});
    registry(4, 3, {0, 1, 1});
    registry(2, 5, {1, 0, 0, 1, 1});
    registry(2, 5, {1, 1, 1, 0, 1}, {-1, -1, 0, -1, 0}); // one key in slots 0, 2 and 4
    registry(2, 8, {1, 1, 1, 1, 1, 1, 1, 1});

    // the rules at their edges, by hand, on a tree of two keys in four positions: entries a < b at positions 0 and 1, Z at 2 and 3
    {
        std::vector<Bytes> h = {Bytes(32, 0x40), Bytes(32, 0x80), Bytes(32, 0), Bytes(32, 0)};
        const Tree t = build(2, 4, h, {1, 1, 0, 0});
        Bytes x(32, 0x60), rec;
        CHECK(prove(t, x, rec) == regsort::KIND_ABSENT && regsort::check_proof(2, 2, x.data(), rec.data(), t.root()) == regsort::KIND_ABSENT);
        // each inequality at equality: the same record for x = h_l and for x = h_r
        CHECK(regsort::check_proof(2, 2, h[0].data(), rec.data(), t.root()) == regsort::KIND_NEITHER);
        CHECK(regsort::check_proof(2, 2, h[1].data(), rec.data(), t.root()) == regsort::KIND_NEITHER);
        // a key leaf claimed as Z, and Z claimed as a key leaf
        Bytes bad = rec;
        bad[regsort::REC_FLAGS] = 3;
        CHECK(regsort::check_proof(2, 2, x.data(), bad.data(), t.root()) == regsort::KIND_NEITHER);
        Bytes y(32, 0x90), ry;
        CHECK(prove(t, y, ry) == regsort::KIND_ABSENT && ry[regsort::REC_FLAGS] == 3 && regsort::check_proof(2, 2, y.data(), ry.data(), t.root()) == regsort::KIND_ABSENT);
        bad = ry;
        bad[regsort::REC_FLAGS] = 7;
        memset(&bad[regsort::REC_H_R], 0xFF, 32);
        CHECK(regsort::check_proof(2, 2, y.data(), bad.data(), t.root()) == regsort::KIND_NEITHER);
        // the left record alone is no proof unless it is the last position
        bad = ry;
        bad[regsort::REC_FLAGS] = 1;
        CHECK(regsort::check_proof(2, 2, y.data(), bad.data(), t.root()) == regsort::KIND_NEITHER);
        // the right record alone is no proof unless it is position 0
        bad = rec;
        bad[regsort::REC_FLAGS] = 6;
        CHECK(regsort::check_proof(2, 2, x.data(), bad.data(), t.root()) == regsort::KIND_NEITHER);
        // stray flag bits, no record at all, bit2 without bit1, PRESENT with a right record
        for (uint32_t f : {0u, 4u, 5u, 8u, 10u, 11u, 15u, 16u | 7u, 0x80000007u}) {
            bad = rec;
            le32_out(&bad[regsort::REC_FLAGS], (int32_t)f);
            CHECK(regsort::check_proof(2, 2, x.data(), bad.data(), t.root()) == regsort::KIND_NEITHER);
        }
        // a PRESENT record for another fingerprint
        Bytes rp;
        CHECK(prove(t, h[1], rp) == regsort::KIND_PRESENT && regsort::check_proof(2, 2, h[1].data(), rp.data(), t.root()) == regsort::KIND_PRESENT);
        CHECK(regsort::check_proof(2, 2, x.data(), rp.data(), t.root()) == regsort::KIND_NEITHER);
        // a full tree: the last key's record has no right half; with a right record claimed, pos_l + 1 == P
        const Tree full = build(2, 2, {h[0], h[1]}, {1, 1});
        CHECK(prove(full, y, ry) == regsort::KIND_ABSENT && ry[regsort::REC_FLAGS] == 1 && regsort::check_proof(2, 1, y.data(), ry.data(), full.root()) == regsort::KIND_ABSENT);
        bad = ry;
        bad[regsort::REC_FLAGS] = 3;
        CHECK(regsort::check_proof(2, 1, y.data(), bad.data(), full.root()) == regsort::KIND_NEITHER);
        // pos_l outside [0, P)
        bad = ry;
        le32_out(&bad[regsort::REC_POS_L], 2);
        CHECK(regsort::check_proof(2, 1, y.data(), bad.data(), full.root()) == regsort::KIND_NEITHER);
        le32_out(&bad[regsort::REC_POS_L], -2);
        CHECK(regsort::check_proof(2, 1, y.data(), bad.data(), full.root()) == regsort::KIND_NEITHER);
    }

    // depth 31: the walk by hand against root_from_path, and a record at the full depth
    {
        Bytes path(31 * 32), h(32);
        fill(path.data(), path.size(), 9);
        fill(h.data(), 32, 10);
        const int32_t poss[3] = {0, 2147483647, 0x2aaaaaaa};
        for (int32_t p : poss) {
            uint8_t cur[32], got[32];
            CHECK(regsort::leaf(3, h.data(), 77, cur) == 0);
            for (int l = 0; l < 31; l++) {
                if ((p >> l) & 1) CHECK(regsort::node(&path[(size_t)l * 32], cur, cur) == 0);
                else CHECK(regsort::node(cur, &path[(size_t)l * 32], cur) == 0);
            }
            CHECK(regsort::root_from_path(3, 31, p, h.data(), 77, path.data(), got) == 0 && !memcmp(got, cur, 32));
            Bytes rec(regsort::proof_bytes(31), 0);
            le32_out(&rec[regsort::REC_POS_L], p);
            le32_out(&rec[regsort::REC_SLOT_L], 77);
            le32_out(&rec[regsort::REC_FLAGS], 9);
            memcpy(&rec[regsort::REC_H_L], h.data(), 32);
            memcpy(&rec[regsort::REC_PATHS], path.data(), path.size());
            CHECK(regsort::check_proof(3, 31, h.data(), rec.data(), cur) == regsort::KIND_PRESENT);
        }
    }

    // refusals
    {
        uint8_t a[32] = {0}, out[32], path[64] = {0};
        Bytes rec(regsort::proof_bytes(1), 0);
        CHECK(regsort::leaf(1, a, 0, out) == -1 && regsort::leaf(5, nullptr, 0, out) == -1 && regsort::leaf(2, a, 0, nullptr) == -1 && regsort::leaf(2, a, -1, out) == -1);
        CHECK(regsort::leaf(2, nullptr, -1, out) == 0);
        CHECK(regsort::node(nullptr, a, out) == -1 && regsort::node(a, nullptr, out) == -1 && regsort::node(a, a, nullptr) == -1);
        CHECK(regsort::root_from_path(1, 1, 0, a, 0, path, out) == -1 && regsort::root_from_path(5, 1, 0, a, 0, path, out) == -1);
        CHECK(regsort::root_from_path(2, -1, 0, a, 0, path, out) == -1 && regsort::root_from_path(2, 32, 0, a, 0, path, out) == -1);
        CHECK(regsort::root_from_path(2, 1, -1, a, 0, path, out) == -1 && regsort::root_from_path(2, 1, 2, a, 0, path, out) == -1);
        CHECK(regsort::root_from_path(2, 1, 0, a, -1, path, out) == -1 && regsort::root_from_path(2, 1, 0, nullptr, -1, path, out) == 0);
        CHECK(regsort::root_from_path(2, 0, 1, a, 0, nullptr, out) == -1 && regsort::root_from_path(2, 0, 0, a, 0, nullptr, out) == 0);
        CHECK(regsort::root_from_path(2, 1, 0, a, 0, nullptr, out) == -1 && regsort::root_from_path(2, 1, 0, a, 0, path, nullptr) == -1);
        CHECK(regsort::check_proof(1, 1, a, rec.data(), a) == -1 && regsort::check_proof(5, 1, a, rec.data(), a) == -1);
        CHECK(regsort::check_proof(2, -1, a, rec.data(), a) == -1 && regsort::check_proof(2, 32, a, rec.data(), a) == -1);
        CHECK(regsort::check_proof(2, 1, nullptr, rec.data(), a) == -1 && regsort::check_proof(2, 1, a, nullptr, a) == -1 && regsort::check_proof(2, 1, a, rec.data(), nullptr) == -1);
        CHECK(regsort::check_proof(2, 1, a, rec.data(), a) == regsort::KIND_NEITHER);
    }
    printf("regsort checks %d failures %d\n", checks, failures);
    return failures ? 1 : 0;
}
