// The host definition of kosk-reghist-v1 (csrc/kosk_reghist.hpp) as a stand-alone program: tests/test_registry_history_host.py builds it
// with ASan + UBSan and runs it.  It builds histories of every size up to 40 from the RECURSIVE definition (written here, independent of the
// header's iterative verifiers), generates every inclusion path and every consistency proof by recursion, and checks that the verifiers
// accept them and reject every truncated, lengthened, altered, mis-headed and badly padded record and every forked old root; then the
// pinned prefixes, unaligned operands and every refusal.  Prints "reghist checks <n> failures 0".
#include <array>
#include <cstdio>
#include <cstring>
#include <vector>

#include "kosk_reghist.hpp"

using namespace kosk;

static int checks = 0, failures = 0;
#define CHECK(x)                                                        \
    do {                                                                \
        checks++;                                                       \
        if (!(x)) { failures++; printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #x); } \
    } while (0)

typedef std::array<uint8_t, 32> Hash;
typedef std::vector<Hash> Hashes;

static void fill(uint8_t *p, size_t n, unsigned seed)
{
    for (size_t i = 0; i < n; i++) p[i] = (uint8_t)(seed = seed * 1103515245u + 12345u, seed >> 16);
}
static Hash N(const Hash &l, const Hash &r)
{
    Hash o;
    CHECK(reghist::node(l.data(), r.data(), o.data()) == 0);
    return o;
}
static int split(int n)
{
    int s = 1;
    while (2 * s < n) s *= 2;
    return s;
}
static Hash mth(const Hash *d, int n)
{
    if (n == 1) return d[0];
    const int s = split(n);
    return N(mth(d, s), mth(d + s, n - s));
}
static void path(const Hash *d, int n, int i, Hashes &out)
{
    if (n == 1) return;
    const int s = split(n);
    if (i < s) { path(d, s, i, out); out.push_back(mth(d + s, n - s)); }
    else { path(d + s, n - s, i - s, out); out.push_back(mth(d, s)); }
}
static void sub(const Hash *d, int n, int m, bool whole, Hashes &out)
{
    if (m == n) { if (!whole) out.push_back(mth(d, n)); return; }
    const int s = split(n);
    if (m <= s) { sub(d, s, m, whole, out); out.push_back(mth(d + s, n - s)); }
    else { sub(d + s, n - s, m - s, false, out); out.push_back(mth(d, s)); }
}
// header, items, zero padding to `bound` items; one spare byte behind it so that an overrun is ASan's to find
static std::vector<uint8_t> pack(const Hashes &items, int w1, int size, int bound)
{
    std::vector<uint8_t> r(16 + 32 * (size_t)bound, 0);
    reghist::le32_out(&r[0], (uint32_t)items.size());
    reghist::le32_out(&r[4], (uint32_t)w1);
    reghist::le32_out(&r[8], (uint32_t)size);
    for (size_t c = 0; c < items.size() && c < (size_t)bound; c++) memcpy(&r[16 + 32 * c], items[c].data(), 32);
    return r;
}

static void histories()
{
    const int MAXN = 40;
    Hashes leaves((size_t)MAXN);
    for (int i = 0; i < MAXN; i++) fill(leaves[(size_t)i].data(), 32, 1000u + (unsigned)i);
    for (int n = 1; n <= MAXN; n++) {
        const Hash root = mth(leaves.data(), n);
        const int D = reghist::depth(n);
        for (int i = 0; i < n; i++) {
            Hashes p;
            path(leaves.data(), n, i, p);
            CHECK((int)p.size() <= D);
            std::vector<uint8_t> rec = pack(p, i, n, D);
            CHECK(rec.size() == reghist::path_bytes(n));
            Hash got;
            CHECK(reghist::root_from_path(i, n, leaves[(size_t)i].data(), rec.data(), got.data()) == 0 && got == root);
            // another index, another leaf
            if (n > 1) {
                std::vector<uint8_t> other = rec;
                reghist::le32_out(&other[4], (uint32_t)((i + 1) % n));
                CHECK(reghist::root_from_path((i + 1) % n, n, leaves[(size_t)i].data(), other.data(), got.data()) != 0 || got != root);
                CHECK(reghist::root_from_path(i, n, leaves[(size_t)((i + 1) % n)].data(), rec.data(), got.data()) == 0 && got != root);
            }
            // the header against the arguments
            CHECK(reghist::root_from_path((i + 1) % (n + 1), n + 1, leaves[(size_t)i].data(), rec.data(), got.data()) == -1 || D != reghist::depth(n + 1));
            std::vector<uint8_t> bad = rec;
            bad[12] = 1;
            CHECK(reghist::root_from_path(i, n, leaves[(size_t)i].data(), bad.data(), got.data()) == -1);
            if (!p.empty()) {
                Hashes q(p.begin(), p.end() - 1); // a record too few
                bad = pack(q, i, n, D);
                CHECK(reghist::root_from_path(i, n, leaves[(size_t)i].data(), bad.data(), got.data()) == -1 || got != root);
                bad = rec; // one altered record
                bad[16 + 32 * (size_t)(i % (int)p.size()) + 5] ^= 0x20;
                CHECK(reghist::root_from_path(i, n, leaves[(size_t)i].data(), bad.data(), got.data()) == 0 && got != root);
            }
            if ((int)p.size() < D) {
                Hashes q = p; // a record too many
                q.push_back(leaves[0]);
                bad = pack(q, i, n, D);
                CHECK(reghist::root_from_path(i, n, leaves[(size_t)i].data(), bad.data(), got.data()) == -1);
                bad = rec; // non-zero padding
                bad[bad.size() - 1] = 1;
                CHECK(reghist::root_from_path(i, n, leaves[(size_t)i].data(), bad.data(), got.data()) == -1);
            }
            bad = rec; // a count above the bound
            reghist::le32_out(&bad[0], (uint32_t)D + 1);
            CHECK(reghist::root_from_path(i, n, leaves[(size_t)i].data(), bad.data(), got.data()) == -1);
        }
        for (int m = 0; m <= n; m++) {
            Hashes p;
            if (0 < m && m < n) sub(leaves.data(), n, m, true, p);
            CHECK((int)p.size() <= D + 1);
            const Hash old = m ? mth(leaves.data(), m) : Hash{};
            std::vector<uint8_t> rec = pack(p, m, n, D + 1);
            CHECK(rec.size() == reghist::consistency_bytes(n));
            CHECK(reghist::check_consistency(m, n, m ? old.data() : nullptr, root.data(), rec.data()) == 1);
            std::vector<uint8_t> bad = rec;
            bad[8] ^= 1; // the header's size
            CHECK(reghist::check_consistency(m, n, old.data(), root.data(), bad.data()) == 0);
            bad = rec;
            bad[4] ^= 1; // the header's old size
            CHECK(reghist::check_consistency(m, n, old.data(), root.data(), bad.data()) == 0);
            bad = rec;
            bad[15] = 0x80;
            CHECK(reghist::check_consistency(m, n, old.data(), root.data(), bad.data()) == 0);
            if ((int)p.size() < D + 1) {
                bad = rec;
                bad[bad.size() - 32] = 1; // non-zero padding
                CHECK(reghist::check_consistency(m, n, old.data(), root.data(), bad.data()) == 0);
                Hashes q = p; // a record too many (for m == 0 and m == n: any record at all)
                q.push_back(p.empty() ? root : p.back());
                bad = pack(q, m, n, D + 1);
                CHECK(reghist::check_consistency(m, n, old.data(), root.data(), bad.data()) == 0);
            }
            bad = rec;
            reghist::le32_out(&bad[0], (uint32_t)D + 2);
            CHECK(reghist::check_consistency(m, n, old.data(), root.data(), bad.data()) == 0);
            if (m == 0) continue;
            Hash forked = old; // a forked old root, another new root
            forked[31] ^= 1;
            CHECK(reghist::check_consistency(m, n, forked.data(), root.data(), rec.data()) == 0);
            if (m < n) {
                CHECK(reghist::check_consistency(m, n, old.data(), forked.data(), rec.data()) == 0);
                Hashes fork(leaves.begin(), leaves.begin() + m); // the old tree with one leaf changed is no prefix
                fork[0][0] ^= 1;
                const Hash fr = mth(fork.data(), m);
                CHECK(reghist::check_consistency(m, n, fr.data(), root.data(), rec.data()) == 0);
                if (!p.empty()) {
                    Hashes q(p.begin(), p.end() - 1);
                    bad = pack(q, m, n, D + 1);
                    CHECK(reghist::check_consistency(m, n, old.data(), root.data(), bad.data()) == 0);
                    bad = rec;
                    bad[16 + 32 * (size_t)(m % (int)p.size())] ^= 1;
                    CHECK(reghist::check_consistency(m, n, old.data(), root.data(), bad.data()) == 0);
                }
            }
        }
    }
}

int main()
{
    CHECK(reghist::depth(0) == 0 && reghist::depth(1) == 0 && reghist::depth(2) == 1 && reghist::depth(3) == 2 && reghist::depth(1025) == 11);
    CHECK(reghist::depth(-1) == -1 && reghist::depth(1 << 24) == 24 && reghist::depth(2147483647) == 31);
    CHECK(reghist::path_bytes(0) == 0 && reghist::path_bytes(-3) == 0 && reghist::path_bytes(1) == 16 && reghist::path_bytes(5) == 16 + 96);
    CHECK(reghist::consistency_bytes(0) == 0 && reghist::consistency_bytes(1) == 48 && reghist::consistency_bytes(5) == 16 + 128);
    CHECK(reghist::nodes_bytes(0) == 0 && reghist::nodes_bytes(1) == 32 && reghist::nodes_bytes(5) == 15 * 32);

    // O begins d8a55b61 / 3bbed6e8 / 5aa09ad7 for kyber_k 2 / 3 / 4; V, C and N of INTEGRATION.md 8.7
    const uint8_t want[3][4] = {{0xd8, 0xa5, 0x5b, 0x61}, {0x3b, 0xbe, 0xd6, 0xe8}, {0x5a, 0xa0, 0x9a, 0xd7}};
    for (int K = 2; K <= 4; K++) {
        uint8_t o[32];
        CHECK(reghist::empty_root(K, o) == 0 && !memcmp(o, want[K - 2], 4));
    }
    {
        uint8_t ev[81] = {0}, out[32], ff[32], z[32] = {0};
        memset(ff, 0xff, 32);
        ev[1] = 1; // at an odd address
        const uint8_t v[4] = {0xa0, 0x72, 0x94, 0x6f}, c[4] = {0xc3, 0xac, 0x69, 0xca}, n[4] = {0xa9, 0x4f, 0xda, 0xf8};
        CHECK(reghist::leaf(3, ev + 1, out) == 0 && !memcmp(out, v, 4));
        ev[1] = 3; ev[1 + 8] = 1; memset(ev + 1 + 48, 0xff, 32);
        CHECK(reghist::leaf(3, ev + 1, out) == 0 && !memcmp(out, c, 4));
        CHECK(reghist::node(z, ff, out) == 0 && !memcmp(out, n, 4));
        // refusals of leaf: k, NULL, the op, every reserved field
        CHECK(reghist::leaf(1, ev + 1, out) == -1 && reghist::leaf(5, ev + 1, out) == -1 && reghist::leaf(3, nullptr, out) == -1 && reghist::leaf(3, ev + 1, nullptr) == -1);
        ev[1] = 0; CHECK(reghist::leaf(3, ev + 1, out) == -1);
        ev[1] = 4; CHECK(reghist::leaf(3, ev + 1, out) == -1);
        ev[1] = 3; ev[1 + 12] = 1; CHECK(reghist::leaf(3, ev + 1, out) == -1);
        ev[1 + 12] = 0; ev[1 + 15] = 0x80; CHECK(reghist::leaf(3, ev + 1, out) == -1);
        ev[1 + 15] = 0; ev[1] = 2; CHECK(reghist::leaf(3, ev + 1, out) == -1); // b and y of an EVICT
        ev[1 + 8] = 0; CHECK(reghist::leaf(3, ev + 1, out) == -1);
        memset(ev + 1 + 48, 0, 32); CHECK(reghist::leaf(3, ev + 1, out) == 0);
        ev[1 + 79] = 1; CHECK(reghist::leaf(3, ev + 1, out) == -1);
        CHECK(reghist::node(nullptr, z, out) == -1 && reghist::node(z, nullptr, out) == -1 && reghist::node(z, z, nullptr) == -1);
        CHECK(reghist::empty_root(1, out) == -1 && reghist::empty_root(5, out) == -1 && reghist::empty_root(2, nullptr) == -1);
    }

    histories();

    // refusals of the verifiers
    {
        uint8_t a[32] = {0}, out[32], rec[48] = {0};
        reghist::le32_out(rec + 8, 1);
        CHECK(reghist::root_from_path(0, 1, a, rec, out) == 0 && !memcmp(out, a, 32));
        CHECK(reghist::root_from_path(0, 0, a, rec, out) == -1 && reghist::root_from_path(-1, 1, a, rec, out) == -1 && reghist::root_from_path(1, 1, a, rec, out) == -1);
        CHECK(reghist::root_from_path(0, 1, nullptr, rec, out) == -1 && reghist::root_from_path(0, 1, a, nullptr, out) == -1 && reghist::root_from_path(0, 1, a, rec, nullptr) == -1);
        CHECK(reghist::check_consistency(0, 1, nullptr, a, rec) == 1);
        CHECK(reghist::check_consistency(-1, 1, a, a, rec) == -1 && reghist::check_consistency(2, 1, a, a, rec) == -1 && reghist::check_consistency(0, 0, a, a, rec) == -1);
        CHECK(reghist::check_consistency(1, 1, nullptr, a, rec) == -1 && reghist::check_consistency(0, 1, a, nullptr, rec) == -1 && reghist::check_consistency(0, 1, a, a, nullptr) == -1);
        reghist::le32_out(rec + 4, 1);
        CHECK(reghist::check_consistency(1, 1, a, a, rec) == 1);
        out[0] = 1;
        CHECK(reghist::check_consistency(1, 1, a, out, rec) == 0);
    }
    printf("reghist checks %d failures %d\n", checks, failures);
    return failures ? 1 : 0;
}
