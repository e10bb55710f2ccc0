// The buffer inventory: every HBM and page-locked host buffer that outlives the call that allocates it is allocated,
// recorded and freed HERE.  One entry says where the buffer's pointer lives (the field the rest of the code reads), how large it is, whether
// it is host or device memory, per proof or whole, which bytes of it can hold secrets, and which owner (group) it comes and goes with.
// wipe_secrets() zeroes the secret spans, secret_scan() searches every entry, release() frees a group, the destructor frees what is left.
//
// Plain C++: memory comes from four function pointers (Ctx fills them with the HIP runtime's, the host test with counting malloc / free).
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace kosk {

// `count` records of `bytes` bytes, `stride` apart (count 1: one run of bytes)
struct WipeRegion { uint8_t *p; size_t bytes, stride; uint32_t count; };

struct InvAlloc { // each returns 0, or the allocator's error code
    int (*dev_alloc)(void **p, size_t bytes);
    int (*dev_free)(void *p);
    int (*host_alloc)(void **p, size_t bytes);
    int (*host_free)(void *p);
};

struct InvBuf {
    const char *name;
    void **at;        // where the buffer's pointer lives; release() sets it to null
    size_t bytes;     // per proof (INV_PER_PROOF) or of the whole buffer; 0: a window whose bytes another entry already lists
    size_t stride;    // INV_PER_PROOF: bytes from one proof's record to the next (what a view is shifted by)
    size_t sec_off, sec_bytes; // the secret part of each record (the key records keep a public head)
    int flags, group;
    bool owned;       // freed by release(); false: a window into another entry's allocation (an alias, every entry of a view)
};

struct Inventory {
    enum { INV_HOST = 1, INV_SECRET = 2, INV_PER_PROOF = 4 };
    enum { INVG_CORE = 0, INVG_VERIFY, INVG_COMPACT, INVG_DENSE, INVG_KEM, INVG_WITNESS, INVG_BIND, INVG_KEMKEY, INVG_FORCE, INVG_TRANSCODE, INVG_BANK, INVG_REGISTRY, INVG_MONITOR, INVG_RELYING, INVG_SIGNER };
    InvAlloc mem{};
    size_t records = 0; // proofs behind every per-proof entry: max_batch of the context that allocates them, own_batch of a view
    std::vector<InvBuf> bufs;

    Inventory() = default;
    Inventory(const Inventory &) = delete; // one owner per allocation
    Inventory &operator=(const Inventory &) = delete;
    ~Inventory() { release_all(); }

    int raw_alloc(void **p, size_t bytes, int flags) const { return (flags & INV_HOST ? mem.host_alloc : mem.dev_alloc)(p, bytes); }
    void raw_free(void *p, int flags) const { if (p) (void)(flags & INV_HOST ? mem.host_free : mem.dev_free)(p); }

    // allocate, store the pointer in *at and own it.  `bytes` per proof x records (INV_PER_PROOF) or whole; alloc_bytes != 0: the allocation
    // is larger than what the entry lists (aliases follow, or an empty table that still gets a valid pointer).  Failure: the allocator's
    // code, *at null, no entry
    template <class T>
    int add(const char *name, T **at, size_t bytes, int flags, int group = INVG_CORE, size_t sec_off = 0, size_t sec_bytes = (size_t)-1, size_t alloc_bytes = 0)
    {
        void *p = nullptr;
        const int e = raw_alloc(&p, alloc_bytes ? alloc_bytes : bytes * (flags & INV_PER_PROOF ? records : 1), flags);
        *at = nullptr;
        if (e) return e;
        adopt(name, at, static_cast<T *>(p), bytes, flags, group, sec_off, sec_bytes);
        return 0;
    }
    // own an allocation that already succeeded (raw_alloc): callers that must keep their old state when filling the new one fails
    template <class T>
    void adopt(const char *name, T **at, T *p, size_t bytes, int flags, int group, size_t sec_off = 0, size_t sec_bytes = (size_t)-1)
    {
        *at = p;
        bufs.push_back(InvBuf{name, reinterpret_cast<void **>(at), bytes, bytes, sec_off, sec_bytes, flags, group, true});
    }
    // a window into an owned entry's allocation: listed (bytes != 0) and shifted in a view like any entry, never freed
    template <class T>
    void alias(const char *name, T **at, T *p, size_t bytes, size_t stride, int flags, int group = INVG_CORE)
    {
        *at = p;
        bufs.push_back(InvBuf{name, reinterpret_cast<void **>(at), bytes, stride, 0, (size_t)-1, flags, group, false});
    }
    // free what the group owns, null every pointer of the group, drop its entries
    void release(int group) { release_if([group](const InvBuf &b) { return b.group == group; }); }
    void release_all() { release_if([](const InvBuf &) { return true; }); }
    template <class F> void release_if(F &&match)
    {
        size_t k = 0;
        for (size_t i = 0; i < bufs.size(); i++) {
            const InvBuf b = bufs[i];
            if (!match(b)) { bufs[k++] = b; continue; }
            if (b.owned) raw_free(*b.at, b.flags);
            *b.at = nullptr;
        }
        bufs.resize(k);
    }
    // this inventory as a view of `arena`: `own` proofs from proof `first` on.  Its entries are the arena's per-proof ones as windows,
    // `first` strides further, their pointers written into `block`, the view's copy of the struct that holds the arena's (`arena_block`).
    // -1: a per-proof pointer of the arena lives outside that struct
    template <class B>
    int view_of(const Inventory &arena, const B &arena_block, B &block, size_t first, size_t own)
    {
        records = own;
        const char *lo = reinterpret_cast<const char *>(&arena_block);
        for (const InvBuf &a : arena.bufs) {
            if (!(a.flags & INV_PER_PROOF)) continue;
            const char *at = reinterpret_cast<const char *>(a.at);
            if (at < lo || at + sizeof(void *) > lo + sizeof(B)) return -1;
            InvBuf b = a;
            b.owned = false;
            b.at = reinterpret_cast<void **>(reinterpret_cast<char *>(&block) + (at - lo));
            *b.at = *a.at ? static_cast<char *>(*a.at) + first * a.stride : nullptr;
            bufs.push_back(b);
        }
        return 0;
    }

    // ---- what the two readers see (kosk_wipe.hip) ----
    // the part of buffer b behind this inventory: nrec records of rec_bytes
    bool span(const InvBuf &b, uint8_t *&p, size_t &rec_bytes, size_t &nrec) const
    {
        p = static_cast<uint8_t *>(*b.at);
        if (!p) return false;
        rec_bytes = b.bytes;
        nrec = (b.flags & INV_PER_PROOF) ? records : 1;
        return rec_bytes != 0;
    }
    // its secret part: the bytes [so, so + sb) of each record
    bool secret_span(const InvBuf &b, uint8_t *&p, size_t &rec, size_t &nrec, size_t &so, size_t &sb) const
    {
        if (!(b.flags & INV_SECRET) || !span(b, p, rec, nrec)) return false;
        so = b.sec_off < rec ? b.sec_off : rec;
        sb = b.sec_bytes < rec - so ? b.sec_bytes : rec - so;
        return sb != 0;
    }
    // the secret device regions (group >= 0: of that owner only; skip_mask: bit g set = not owner g's)
    int secret_regions(std::vector<WipeRegion> &out, int group = -1, unsigned skip_mask = 0) const
    {
        for (const InvBuf &b : bufs) {
            uint8_t *p;
            size_t rec, nrec, so, sb;
            if ((group >= 0 && b.group != group) || (skip_mask >> b.group & 1) || (b.flags & INV_HOST) || !secret_span(b, p, rec, nrec, so, sb)) continue;
            // records without a public part lie back to back: one record of nrec x rec bytes
            if (so == 0 && sb == rec) out.push_back(WipeRegion{p, rec * nrec, 0, 1});
            else out.push_back(WipeRegion{p + so, sb, rec, (uint32_t)nrec});
        }
        return (int)out.size();
    }
};

} // namespace kosk
