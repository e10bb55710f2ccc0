// Stand-alone check of csrc/kosk_inventory.hpp on counting malloc / free: built with ASan + UBSan and run as a child
// process by tests/test_inventory_host.py.  Every property is asserted with the counters below, so the result does not depend on a leak
// checker.  Prints "inventory checks N failures 0" and exits 0, or names every failed check and exits 1.
#include "kosk_inventory.hpp"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <string>

using namespace kosk;

// ---- the allocator: every block is known by kind; a free of anything else (an alias, a second free) is counted as a fault ----
static std::map<void *, int> g_live; // pointer -> 0 device, 1 host
static long g_allocs = 0, g_frees = 0, g_bad_frees = 0, g_fail_at = 0; // g_fail_at = k > 0: the k-th allocation from now fails
static int g_failures = 0, g_checks = 0;

static int alloc_kind(void **p, size_t bytes, int kind)
{
    if (g_fail_at > 0 && --g_fail_at == 0) { *p = nullptr; return 2; } // "out of memory"
    *p = malloc(bytes ? bytes : 1);
    g_live[*p] = kind;
    g_allocs++;
    return 0;
}
static int free_kind(void *p, int kind)
{
    auto it = g_live.find(p);
    if (it == g_live.end() || it->second != kind) { g_bad_frees++; return 1; }
    g_live.erase(it);
    free(p);
    g_frees++;
    return 0;
}
static void wire(Inventory &v)
{
    v.mem.dev_alloc = [](void **p, size_t n) { return alloc_kind(p, n, 0); };
    v.mem.dev_free = [](void *p) { return free_kind(p, 0); };
    v.mem.host_alloc = [](void **p, size_t n) { return alloc_kind(p, n, 1); };
    v.mem.host_free = [](void *p) { return free_kind(p, 1); };
}

#define CHECK(x)                                                                 \
    do {                                                                         \
        g_checks++;                                                              \
        if (!(x)) { g_failures++; printf("FAILED %s:%d  %s\n", __FILE__, __LINE__, #x); } \
    } while (0)

enum { HOST = Inventory::INV_HOST, SEC = Inventory::INV_SECRET, PP = Inventory::INV_PER_PROOF };

static std::string listing(const Inventory &v) // everything of the entries but the addresses
{
    std::string s;
    for (const InvBuf &b : v.bufs) {
        char line[256];
        snprintf(line, sizeof line, "%s %zu %zu %zu %zu %d %d %d\n", b.name, b.bytes, b.stride, b.sec_off, b.sec_bytes, b.flags, b.group, (int)b.owned);
        s += line;
    }
    return s;
}

// ---- 1. five buffers over three groups; releasing the middle one ----
static void check_groups()
{
    uint8_t *a = nullptr, *b = nullptr, *c = nullptr, *e = nullptr; // (the pointers outlive the inventory that writes to them)
    uint32_t *d = nullptr;
    Inventory v;
    wire(v);
    const long a0 = g_allocs, f0 = g_frees;
    CHECK(v.add("a", &a, 100, 0, 0) == 0 && v.add("b", &b, 50, HOST, 0) == 0);
    CHECK(v.add("c", &c, 70, SEC, 1) == 0 && v.add("d", &d, 16, HOST, 1) == 0);
    CHECK(v.add("e", &e, 9, 0, 2) == 0);
    CHECK(g_allocs - a0 == 5 && a && b && c && d && e && v.bufs.size() == 5);
    void *pc = c, *pd = d;
    v.release(1);
    CHECK(g_frees - f0 == 2 && !g_live.count(pc) && !g_live.count(pd)); // exactly its two allocations
    CHECK(!c && !d && a && b && e);                                       // exactly its owners' pointers
    CHECK(g_live.count(a) && g_live.count(b) && g_live.count(e) && v.bufs.size() == 3);
    CHECK(listing(v) == "a 100 100 0 18446744073709551615 0 0 1\nb 50 50 0 18446744073709551615 1 0 1\ne 9 9 0 18446744073709551615 0 2 1\n");
    v.release(1); // nothing left of it: a no-op
    CHECK(g_frees - f0 == 2 && v.bufs.size() == 3);
    v.release_all();
    CHECK(g_frees - f0 == 5 && !a && !b && !e && v.bufs.empty() && g_bad_frees == 0);
}

// ---- 2. an `ensure` of four buffers that fails at its k-th allocation, for every k ----
struct Ws { uint8_t *p[4] = {nullptr, nullptr, nullptr, nullptr}; }; // sk, salt, ok, h_ok
static int ensure(Inventory &v, Ws &w, size_t n)
{
    int e;
    if ((e = v.add("sk", &w.p[0], n * 1632, SEC, 5))) return e;
    if ((e = v.add("salt", &w.p[1], n * 32, SEC, 5))) return e;
    if ((e = v.add("ok", &w.p[2], n, 0, 5))) return e;
    if ((e = v.add("h_ok", &w.p[3], n, HOST, 5))) return e;
    return 0;
}
static void check_failure_injection()
{
    std::string first_try;
    {
        Ws w;
        Inventory v;
        wire(v);
        CHECK(ensure(v, w, 3) == 0);
        first_try = listing(v);
    }
    for (int k = 1; k <= 4; k++) {
        uint8_t *core = nullptr;
        Ws w;
        Inventory v;
        wire(v);
        CHECK(v.add("core", &core, 8, 0, 0) == 0); // another group's buffer stays through all of it
        const long a0 = g_allocs, f0 = g_frees;
        g_fail_at = k;
        CHECK(ensure(v, w, 3) == 2);
        CHECK(g_fail_at == 0 && g_allocs - a0 == k - 1);
        CHECK(w.p[k - 1] == nullptr && v.bufs.size() == (size_t)k); // the failed add: pointer null, no entry (core + k - 1 entries)
        v.release(5); // what the caller does before it returns the error
        CHECK(v.bufs.size() == 1 && !w.p[0] && !w.p[1] && !w.p[2] && !w.p[3] && core);
        CHECK(g_allocs - a0 == g_frees - f0 && g_bad_frees == 0);
        CHECK(ensure(v, w, 3) == 0 && w.p[0] && w.p[1] && w.p[2] && w.p[3]); // the retry starts from nothing
        CHECK(listing(v) == "core 8 8 0 18446744073709551615 0 0 1\n" + first_try);
    }
}

// ---- 3. an arena of 6 proofs and a view of proofs 2..3; 5. the secret regions of both ----
// the key record of K = 2 as ctx_create lays it out: [pk 800 | NTT(s) 768 | seeds 64], the head public
enum { PKPAD = 800, KG_REC = 800 + 768 + 64, SEL = 2624 };
struct Block { uint8_t *P = nullptr, *kg = nullptr, *h_kg = nullptr, *pk = nullptr, *sb = nullptr, *I = nullptr, *rest = nullptr, *h_tape = nullptr, *dig = nullptr; };
struct Owner { uint8_t *table = nullptr, *h_err = nullptr, *key = nullptr; };

// kosk_wipe.hip's arithmetic (inv_span, inv_secret_span, wipe_regions_list) for one secret device entry whose pointer is p
static WipeRegion parent_region(uint8_t *p, size_t bytes, size_t sec_off, size_t sec_bytes, bool per_proof, bool is_view, size_t own_batch, size_t max_batch)
{
    const size_t rec = bytes, nrec = per_proof ? (is_view ? own_batch : max_batch) : 1;
    const size_t so = sec_off < rec ? sec_off : rec;
    const size_t sb = sec_bytes < rec - so ? sec_bytes : rec - so;
    if (so == 0 && sb == rec) return WipeRegion{p, rec * nrec, 0, 1};
    return WipeRegion{p + so, sb, rec, (uint32_t)nrec};
}
static bool same(const WipeRegion &a, const WipeRegion &b) { return a.p == b.p && a.bytes == b.bytes && a.stride == b.stride && a.count == b.count; }

static int fill_arena(Inventory &v, Block &b, Owner &o, size_t B)
{
    v.records = B;
    int e = 0;
    e |= v.add("table", &o.table, 4096, 0);
    e |= v.add("d_P", &b.P, 64, PP | SEC);
    e |= v.add("d_kg", &b.kg, KG_REC, PP | SEC, 0, PKPAD, KG_REC - PKPAD);
    e |= v.add("h_kg", &b.h_kg, KG_REC, PP | HOST | SEC, 0, PKPAD, KG_REC - PKPAD);
    if (e) return e;
    v.alias("d_pk", &b.pk, b.kg, 0, KG_REC, PP);         // windows that list no bytes of their own
    v.alias("d_sb", &b.sb, b.kg + PKPAD, 0, KG_REC, PP);
    e |= v.add("d_I", &b.I, SEL, PP, 0, 0, (size_t)-1, 2 * B * SEL); // two halves in one allocation
    if (e) return e;
    v.alias("d_rest", &b.rest, b.I + B * SEL, SEL, SEL, PP);
    e |= v.add("h_tape", &b.h_tape, 128, PP | HOST | SEC);
    e |= v.add("workspace", &b.dig, 32, PP);
    e |= v.add("h_err", &o.h_err, 64, HOST);
    e |= v.add("kemkey.sec", &o.key, 800, SEC, Inventory::INVG_KEMKEY);
    return e;
}

static void check_arena_and_view()
{
    const size_t B = 6, first = 2, own = 2;
    const long a0 = g_allocs, f0 = g_frees;
    {
        Block ab;
        Owner ao;
        Inventory arena;
        wire(arena);
        CHECK(fill_arena(arena, ab, ao, B) == 0);
        CHECK(g_allocs - a0 == 9 && arena.bufs.size() == 12);
        CHECK(ab.pk == ab.kg && ab.sb == ab.kg + PKPAD && ab.rest == ab.I + B * SEL);

        // the owner's secret regions: max_batch records each; host entries and public ones are not among them
        std::vector<WipeRegion> r;
        CHECK(arena.secret_regions(r) == 3 && r.size() == 3);
        CHECK(same(r[0], WipeRegion{ab.P, 64 * 6, 0, 1}) && same(r[0], parent_region(ab.P, 64, 0, (size_t)-1, true, false, B, B)));
        CHECK(same(r[1], WipeRegion{ab.kg + 800, 832, 1632, 6}) && same(r[1], parent_region(ab.kg, KG_REC, PKPAD, KG_REC - PKPAD, true, false, B, B)));
        CHECK(same(r[2], WipeRegion{ao.key, 800, 0, 1}) && same(r[2], parent_region(ao.key, 800, 0, (size_t)-1, false, false, B, B)));
        r.clear();
        CHECK(arena.secret_regions(r, Inventory::INVG_KEMKEY) == 1 && same(r[0], WipeRegion{ao.key, 800, 0, 1}));
        r.clear();
        CHECK(arena.secret_regions(r, -1, 1u << Inventory::INVG_KEMKEY | 1u << Inventory::INVG_BANK) == 2 && r[1].p == ab.kg + 800);
        { // the host reader's span of the key record's mirror, and a window without bytes is no span at all
            uint8_t *p;
            size_t rec, nrec, so, sb;
            CHECK(arena.secret_span(arena.bufs[3], p, rec, nrec, so, sb) && p == ab.h_kg && rec == 1632 && nrec == 6 && so == 800 && sb == 832);
            CHECK(!arena.span(arena.bufs[4], p, rec, nrec));
            CHECK(arena.span(arena.bufs[7], p, rec, nrec) && p == ab.rest && rec == SEL && nrec == 6);
        }

        const long a1 = g_allocs, f1 = g_frees;
        {
            Block vb;
            uint8_t *mine = nullptr, *h_err = nullptr;
            Inventory view;
            wire(view);
            CHECK(view.view_of(arena, ab, vb, first, own) == 0);
            CHECK(g_allocs == a1 && view.records == own);
            // the per-proof entries only (not table, h_err, the key), none owned, each at base + 2 strides
            CHECK(view.bufs.size() == 9);
            CHECK(listing(view) == "d_P 64 64 0 18446744073709551615 6 0 0\nd_kg 1632 1632 800 832 6 0 0\nh_kg 1632 1632 800 832 7 0 0\n"
                                   "d_pk 0 1632 0 18446744073709551615 4 0 0\nd_sb 0 1632 0 18446744073709551615 4 0 0\n"
                                   "d_I 2624 2624 0 18446744073709551615 4 0 0\nd_rest 2624 2624 0 18446744073709551615 4 0 0\n"
                                   "h_tape 128 128 0 18446744073709551615 7 0 0\nworkspace 32 32 0 18446744073709551615 4 0 0\n");
            CHECK(vb.P == ab.P + 2 * 64 && vb.kg == ab.kg + 2 * 1632 && vb.h_kg == ab.h_kg + 2 * 1632 && vb.pk == ab.pk + 2 * 1632);
            CHECK(vb.sb == ab.sb + 2 * 1632 && vb.I == ab.I + 2 * SEL && vb.rest == ab.rest + 2 * SEL && vb.h_tape == ab.h_tape + 2 * 128 && vb.dig == ab.dig + 2 * 32);
            for (const InvBuf &e : view.bufs) CHECK(reinterpret_cast<char *>(e.at) >= reinterpret_cast<char *>(&vb) && reinterpret_cast<char *>(e.at) < reinterpret_cast<char *>(&vb + 1));
            // the view's regions: own_batch records of its block
            CHECK(view.secret_regions(r = {}) == 2);
            CHECK(same(r[0], WipeRegion{ab.P + 128, 64 * 2, 0, 1}) && same(r[0], parent_region(vb.P, 64, 0, (size_t)-1, true, true, own, B - first)));
            CHECK(same(r[1], WipeRegion{ab.kg + 2 * 1632 + 800, 832, 1632, 2}) && same(r[1], parent_region(vb.kg, KG_REC, PKPAD, KG_REC - PKPAD, true, true, own, B - first)));
            // what the view allocates itself comes and goes with it
            CHECK(view.add("h_err", &h_err, 64, HOST) == 0 && view.add("d_wsk", &mine, 1632, SEC, Inventory::INVG_WITNESS) == 0);
            CHECK(g_allocs - a1 == 2 && view.bufs.size() == 11 && view.secret_regions(r = {}) == 3 && same(r[2], WipeRegion{mine, 1632, 0, 1}));
            view.release(Inventory::INVG_WITNESS);
            CHECK(!mine && g_frees - f1 == 1 && view.bufs.size() == 10);
        } // the view goes: its h_err, and nothing of the arena's
        CHECK(g_frees - f1 == 2 && g_allocs - a1 == 2 && g_bad_frees == 0);
        CHECK(g_live.count(ab.P) && g_live.count(ab.kg) && g_live.count(ab.h_kg) && g_live.count(ab.I) && g_live.count(ab.h_tape) && g_live.count(ab.dig));
        CHECK(ab.P && ab.rest && ab.pk); // the arena's pointers are untouched

        // a per-proof pointer outside the block is refused
        Block sb2;
        Owner so2;
        Inventory stray, bad;
        wire(stray);
        wire(bad);
        bad.records = B;
        CHECK(bad.add("outside", &so2.table, 8, PP) == 0 && stray.view_of(bad, ab, sb2, 1, 1) == -1);
    } // the arena goes: every allocation once, the aliases never
    CHECK(g_allocs - a0 == g_frees - f0 && g_bad_frees == 0);
}

// ---- 4. adopt, then release ----
static void check_adopt()
{
    uint8_t *armed = nullptr, *d = nullptr;
    Inventory v;
    wire(v);
    const long a0 = g_allocs, f0 = g_frees;
    CHECK(v.raw_alloc(reinterpret_cast<void **>(&d), 96, 0) == 0 && d && v.bufs.empty()); // filled by the caller; a failure there: raw_free, old state kept
    v.adopt("d_contexts", &armed, d, 96, 0, Inventory::INVG_BIND);
    CHECK(armed == d && v.bufs.size() == 1 && v.bufs[0].owned && v.bufs[0].bytes == 96 && v.bufs[0].group == Inventory::INVG_BIND);
    v.release(Inventory::INVG_BIND);
    CHECK(!armed && v.bufs.empty() && g_allocs - a0 == 1 && g_frees - f0 == 1 && g_bad_frees == 0);
    uint8_t *t = nullptr;
    CHECK(v.raw_alloc(reinterpret_cast<void **>(&t), 8, HOST) == 0);
    v.raw_free(t, HOST);
    v.raw_free(nullptr, 0);
    CHECK(g_allocs - a0 == 2 && g_frees - f0 == 2 && g_bad_frees == 0);
}

int main()
{
    check_groups();
    check_failure_injection();
    check_arena_and_view();
    check_adopt();
    CHECK(g_live.empty() && g_allocs == g_frees && g_bad_frees == 0);
    printf("inventory checks %d failures %d\n", g_checks, g_failures);
    return g_failures ? 1 : 0;
}
