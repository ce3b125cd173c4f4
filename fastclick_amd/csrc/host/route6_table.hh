// route6_table.hh -- the IPv6 route table of FCGPU_CLS_ROUTE6, built on the host.
//
// Semantics: LookupIP6Route behind GetIP6Address(24) (elements/ip6/
// lookupip6route.cc:98-149, lib/ip6table.cc:32-73): routes are addr/plen [gw]
// port with addr &= mask, lookup returns the longest matching prefix, and a
// second route for one addr/plen replaces the first (IP6Table::add deletes,
// then adds) -- unlike IPv4's "conflict with existing route". Only contiguous
// masks (prefix lengths 0..128) are supported. The gateway of a next hop is a
// gateway id, not an address: 0 = no gateway (::), else 1 + the position of
// the route's gateway among the distinct non-zero gateways in order of first
// appearance in the route list as given (overridden routes included).
//
// Structure: a path-compressed, leaf-pushed 16-8-...-8 trie of
// 32-bit entries, laid out for a GPU lane that pays one L2 round trip per
// dependent load:
//   root[65536]      indexed by address bytes 0..1 (256 KB);
//   chunk k          260 words = 1040 B: a 16-byte header, then 256 entries
//                    indexed by one address byte.
// An entry with bit 31 clear is a leaf: a next-hop index, 0 = no route. With
// bit 31 set, bits 30..27 are `skip` (0..13 address bytes stepped over before
// the chunk's index byte) and bits 26..0 the chunk. A chunk in which no route
// ends and which has one child is not emitted: its index byte joins the
// child's skipped bytes, and the leaf all its other slots would have held (the
// leaf inherited from above) is the child's *default leaf*. The header holds
// the default leaf in bytes 0..1 and each skipped address byte at its own
// position in the address (bytes 2..14; the root consumed 0..1 and the last
// byte is always an index). That differs from "skipped bytes first, default
// last" on purpose: header and key then line up word for word, so the walk
// compares them with four masked 32-bit xors and no shifting, whatever the
// depth. The parent entry gives both the header's and the entry's address, so
// a walk issues them together: one round trip per surviving chunk.
//
// Bounds, for any 128-bit key: the builder writes every word of the image. A
// chunk entry is written only by emit(), which names the chunk it has just
// appended (index < nchunks) and a skip with depth + skip <= 15, so the index
// byte is one of the key's 16; a leaf is a next-hop index the builder
// allocated (< hops.size() <= 32768), and so is every default leaf. The walk
// moves at least one byte deeper per chunk and ends at byte 15 at the latest.
//
// Size: 256 KB + 1040 B per surviving chunk + 8 B per next hop, refused above
// kMaxImageBytes (256 MiB: about 258,000 chunks, far below the 2^27 the
// encoding could name; hop_off stays a 32-bit byte offset).
//
// No HIP here: the library (fcgpu_set_routes6), fcgpu_route6_lookup /
// fcgpu_route6_stats and CPU programs share this file.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>
#include "../../../include/fastclick_gpu.h"

namespace fcroute6 {

constexpr uint32_t kLeafMax = 0x7fff;        // next hops 1 .. kLeafMax
constexpr uint32_t kChunkBit = 0x80000000u;
constexpr uint32_t kChunkMask = 0x07ffffffu;
constexpr uint32_t kChunkWords = 260;        // 4 header words + 256 entries
constexpr uint32_t kRootWords = 65536;
constexpr uint32_t kNoPort = 0xffffffffu;    // next hop 0's port: no route
constexpr size_t kMaxImageBytes = (size_t)256 << 20;

struct NextHop {
    uint32_t gw_id;   // 0 = the destination is the next hop
    uint32_t port;
};

struct Table {
    std::vector<uint32_t> root;     // 65536 entries
    std::vector<uint32_t> chunks;   // kChunkWords per chunk
    std::vector<NextHop> hops;      // [0] = {0, kNoPort}
    uint32_t max_port = 0;          // largest output of any route
    uint32_t max_loads = 1;         // longest walk: the root load + one per chunk on the path
    uint32_t nchunks() const { return (uint32_t)(chunks.size() / kChunkWords); }
    size_t image_bytes() const { return (root.size() + chunks.size()) * 4 + ((hops.size() * 8 + 15) & ~(size_t)15); }
};

namespace detail {
struct R {
    uint8_t a[16];
    uint32_t hop;
    uint32_t plen;
};
struct Builder {
    Table &t;
    const std::vector<R> &rs;
    bool full = false;

    // Controlled prefix expansion of the routes `ends` (all ending in the 256
    // slots at `at`, i.e. 8 * d < plen <= 8 * d + 8) in ascending length.
    void expand(std::vector<uint32_t> &ends, size_t at, uint32_t d) {
        std::stable_sort(ends.begin(), ends.end(), [&](uint32_t x, uint32_t y) { return rs[x].plen < rs[y].plen; });
        for (uint32_t k : ends)
            std::fill_n(t.chunks.begin() + at + rs[k].a[d], 1u << (8 * d + 8 - rs[k].plen), rs[k].hop);
    }
    // The entry for the routes `ix` (sorted by address, sharing bytes [0, d),
    // every plen > 8 * d) below a slot that so far held the leaf `inh`.
    uint32_t emit(const std::vector<uint32_t> &ix, uint32_t d, uint32_t inh, uint32_t loads) {
        const uint32_t d0 = d;
        for (;; ++d) {    // path compression: no route ends at byte d and all go the same way
            bool ends = false;
            for (uint32_t k : ix) ends |= rs[k].plen <= 8 * d + 8;
            if (ends || rs[ix.front()].a[d] != rs[ix.back()].a[d]) break;
        }
        // a /128 ends at d = 15 at the latest, so d <= 15 and skip <= 13
        const uint32_t c = t.nchunks();
        if (t.image_bytes() + kChunkWords * 4 > kMaxImageBytes || c >= kChunkMask) {
            full = true;
            return inh;
        }
        t.max_loads = std::max(t.max_loads, loads + 1);
        const size_t at = (size_t)c * kChunkWords;
        t.chunks.resize(at + kChunkWords, inh);
        uint8_t hdr[16] = {(uint8_t)inh, (uint8_t)(inh >> 8)};
        for (uint32_t j = d0; j < d; ++j) hdr[j] = rs[ix.front()].a[j];
        memcpy(&t.chunks[at], hdr, 16);
        std::vector<uint32_t> ends, kid;
        for (uint32_t k : ix)
            if (rs[k].plen <= 8 * d + 8) ends.push_back(k);
        expand(ends, at + 4, d);
        for (size_t i = 0; i < ix.size() && !full;) {     // children: runs of one index byte, longer prefixes only
            const uint32_t b = rs[ix[i]].a[d];
            kid.clear();
            for (; i < ix.size() && rs[ix[i]].a[d] == b; ++i)
                if (rs[ix[i]].plen > 8 * d + 8) kid.push_back(ix[i]);
            if (kid.empty()) continue;
            const uint32_t e = emit(kid, d + 1, t.chunks[at + 4 + b], loads + 1);   // may grow t.chunks
            t.chunks[at + 4 + b] = e;
        }
        return kChunkBit | ((d - d0) << 27) | c;
    }
};
}  // namespace detail

// Build the trie. nports 0: outputs are not bounded here (the submission
// checks max_port). Returns FCGPU_OK or FCGPU_EINVAL with `err` set.
inline int build(const fcgpu_route6 *routes, uint32_t n, uint32_t nports, Table &t, std::string &err) {
    using detail::R;
    static const uint8_t zero[16] = {0};
    t.root.assign(kRootWords, 0);
    t.chunks.clear();
    t.hops.assign(1, NextHop{0, kNoPort});
    t.max_port = 0;
    t.max_loads = 1;
    std::map<std::vector<uint8_t>, uint32_t> gw_id;               // gateway -> id, first appearance
    std::map<std::vector<uint8_t>, std::pair<uint32_t, uint32_t>> last;   // addr + plen -> (gw id, port): last wins
    std::vector<std::vector<uint8_t>> order;                      // keys of `last` in order of first appearance
    for (uint32_t k = 0; k < n; ++k) {
        const fcgpu_route6 &r = routes[k];
        if (r.plen > 128) { err = "route " + std::to_string(k) + ": prefix length > 128"; return FCGPU_EINVAL; }
        if (r.port >= FCGPU_MAX_PORTS || (nports && r.port >= nports)) {
            err = "route " + std::to_string(k) + ": bad OUTPUT";
            return FCGPU_EINVAL;
        }
        uint32_t g = 0;
        if (memcmp(r.gw, zero, 16)) {
            const std::vector<uint8_t> gk(r.gw, r.gw + 16);
            g = gw_id.emplace(gk, (uint32_t)gw_id.size() + 1).first->second;
        }
        std::vector<uint8_t> key(17, 0);
        for (uint32_t j = 0; j < 16; ++j) {          // addr &= mask
            const int bits = (int)r.plen - 8 * (int)j;
            key[j] = bits >= 8 ? r.addr[j] : bits <= 0 ? 0 : (uint8_t)(r.addr[j] & (0xff00u >> bits));
        }
        key[16] = r.plen;
        auto ins = last.emplace(key, std::make_pair(g, (uint32_t)r.port));
        if (ins.second) order.push_back(key);
        else ins.first->second = std::make_pair(g, (uint32_t)r.port);
        t.max_port = std::max(t.max_port, (uint32_t)r.port);
    }
    std::vector<R> rs;
    rs.reserve(last.size());
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> hop_of;     // (gw id, port) -> index
    for (const auto &key : order) {
        const auto gp = last[key];
        auto it = hop_of.find(gp);
        if (it == hop_of.end()) {
            if (t.hops.size() > kLeafMax) { err = "more than 32767 next hops"; return FCGPU_EINVAL; }
            it = hop_of.emplace(gp, (uint32_t)t.hops.size()).first;
            t.hops.push_back(NextHop{gp.first, gp.second});
        }
        R r;
        memcpy(r.a, key.data(), 16);
        r.hop = it->second;
        r.plen = key[16];
        rs.push_back(r);
    }
    // the root: prefixes up to /16 expanded in ascending length, then one
    // subtree per 16-bit slot that longer prefixes pass through
    std::vector<uint32_t> ix(rs.size());
    for (uint32_t k = 0; k < ix.size(); ++k) ix[k] = k;
    std::stable_sort(ix.begin(), ix.end(), [&](uint32_t x, uint32_t y) {
        const int c = memcmp(rs[x].a, rs[y].a, 16);
        return c ? c < 0 : rs[x].plen < rs[y].plen;
    });
    std::vector<uint32_t> shorts;
    for (uint32_t k : ix)
        if (rs[k].plen <= 16) shorts.push_back(k);
    std::stable_sort(shorts.begin(), shorts.end(), [&](uint32_t x, uint32_t y) { return rs[x].plen < rs[y].plen; });
    for (uint32_t k : shorts)
        std::fill_n(t.root.begin() + (rs[k].a[0] << 8 | rs[k].a[1]), 1u << (16 - rs[k].plen), rs[k].hop);
    detail::Builder b{t, rs};
    std::vector<uint32_t> kid;
    for (size_t i = 0; i < ix.size() && !b.full;) {
        const uint32_t top = rs[ix[i]].a[0] << 8 | rs[ix[i]].a[1];
        kid.clear();
        for (; i < ix.size() && (uint32_t)(rs[ix[i]].a[0] << 8 | rs[ix[i]].a[1]) == top; ++i)
            if (rs[ix[i]].plen > 16) kid.push_back(ix[i]);
        if (!kid.empty()) t.root[top] = b.emit(kid, 2, t.root[top], 1);
    }
    if (b.full) {
        err = "route table image larger than " + std::to_string(kMaxImageBytes >> 20) + " MiB";
        return FCGPU_EINVAL;
    }
    return FCGPU_OK;
}

// Byte [lo, hi) of an address as a mask over its word j (little-endian words)
inline uint32_t word_mask(int lo, int hi, int j) {
    const int a = std::min(std::max(lo - 4 * j, 0), 4), b = std::min(std::max(hi - 4 * j, 0), 4);
    return (uint32_t)(((uint64_t)1 << (8 * b)) - 1) & ~(uint32_t)(((uint64_t)1 << (8 * a)) - 1);
}

// The walk, exactly as the device does it (fcgpu_device.hh route6_walk).
// key: the 16 address bytes. Returns the next-hop index (0 = no route).
inline uint32_t walk(const uint32_t *root, const uint32_t *chunks, const uint8_t key[16]) {
    uint32_t k[4];
    memcpy(k, key, 16);
    uint32_t e = root[key[0] << 8 | key[1]], d = 2;
    while (e & kChunkBit) {
        const uint32_t skip = (e >> 27) & 15;
        const uint32_t *ch = chunks + (size_t)(e & kChunkMask) * kChunkWords;
        uint32_t diff = 0;
        for (int j = 0; j < 4 && skip; ++j) diff |= (ch[j] ^ k[j]) & word_mask((int)d, (int)(d + skip), j);
        if (diff) return ch[0] & 0xffff;
        d += skip;
        e = ch[4 + key[d & 15]];
        ++d;
    }
    return e;
}

// LookupIP6Route: the output port or -1; *gw_id (may be null) gets the
// route's gateway id, 0 when it has none.
inline int lookup(const Table &t, const uint8_t key[16], uint32_t *gw_id) {
    const NextHop &h = t.hops[walk(t.root.data(), t.chunks.data(), key)];
    if (gw_id) *gw_id = h.port == kNoPort ? 0u : h.gw_id;
    return h.port == kNoPort ? -1 : (int)h.port;
}

// The device image: root, the chunks, then the next hops (8 B each, padded to
// 16 B so a workgroup can stage them with whole uint4 loads). hop_off = the
// byte offset of the next hops, a multiple of 16.
inline std::vector<uint8_t> image(const Table &t, uint32_t &hop_off) {
    hop_off = (uint32_t)((t.root.size() + t.chunks.size()) * 4);
    std::vector<uint8_t> img(t.image_bytes(), 0);
    memcpy(img.data(), t.root.data(), t.root.size() * 4);
    if (!t.chunks.empty()) memcpy(img.data() + t.root.size() * 4, t.chunks.data(), t.chunks.size() * 4);
    memcpy(img.data() + hop_off, t.hops.data(), t.hops.size() * sizeof(NextHop));
    return img;
}

}  // namespace fcroute6
