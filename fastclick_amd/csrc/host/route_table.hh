// route_table.hh -- the IPv4 route table of FCGPU_CLS_ROUTE, built on the host.
//
// Semantics: IPRouteTable (elements/ip/iproutetable.cc:35-60,152-169): routes
// are addr/mask [gw] port with addr &= mask, a second route for one addr/plen
// is a conflict, and lookup_route returns the longest matching prefix's
// (port, gw) or -1.
//
// Structure: a leaf-pushed 16-8-8 multibit trie of 16-bit
// entries, not the reference's 32-MB DIR-24-8 arrays (directiplookup.hh):
//   l0[65536]        indexed by the top 16 bits of the host-order address;
//   chunks[k][256]   a shared pool, indexed by the next address byte.
// An entry < 0x8000 is a leaf: a next-hop index, 0 = no route. An entry
// >= 0x8000 names chunk (entry & 0x7fff). Second-level chunk entries use the
// same encoding, third-level entries are leaves. Next hops are the distinct
// (gw, port) pairs, as DirectIPLookup's vports (directiplookup.cc:133-156).
// Every entry is written by the builder below, so for any 32-bit key every
// index of the walk is in range: a chunk entry names a chunk that exists and
// a leaf names a next hop that exists.
//
// No HIP here: the library (fcgpu_set_routes), fcgpu_route_lookup and CPU
// programs share this file.
#pragma once
#include <stdint.h>
#include <algorithm>
#include <map>
#include <string>
#include <utility>
#include <vector>
#include "../../../include/fastclick_gpu.h"

namespace fcroute {

constexpr uint32_t kLeafMax = 0x7fff;      // next hops 1 .. kLeafMax, chunks 0 .. kLeafMax - 1
constexpr uint16_t kChunkBit = 0x8000;
constexpr uint32_t kNoPort = 0xffffffffu;  // next hop 0's port: no route

struct NextHop {
    uint32_t gw;      // raw network order, 0 = keep the packet's address
    uint32_t port;
};

struct Table {
    std::vector<uint16_t> l0;       // 65536 entries
    std::vector<uint16_t> chunks;   // 256 entries per chunk
    std::vector<NextHop> hops;      // [0] = {0, kNoPort}
    uint32_t max_port = 0;          // largest output of any route
    uint32_t nchunks() const { return (uint32_t)(chunks.size() >> 8); }
};

inline uint32_t host_order(uint32_t raw) { return __builtin_bswap32(raw); }   // raw = little-endian load of the bytes

// Build the trie. nports 0: outputs are not bounded here (the submission
// checks max_port). Returns FCGPU_OK or FCGPU_EINVAL with `err` set.
inline int build(const fcgpu_route *routes, uint32_t n, uint32_t nports, Table &t, std::string &err) {
    struct R { uint32_t addr, hop; uint8_t plen; };
    std::vector<R> rs;
    rs.reserve(n);
    t.l0.assign(65536, 0);
    t.chunks.clear();
    t.hops.assign(1, NextHop{0, kNoPort});
    t.max_port = 0;
    std::map<std::pair<uint32_t, uint32_t>, uint32_t> hop_of;    // (gw, port) -> index
    for (uint32_t k = 0; k < n; ++k) {
        const fcgpu_route &r = routes[k];
        if (r.plen > 32) { err = "route " + std::to_string(k) + ": prefix length > 32"; return FCGPU_EINVAL; }
        if (r.port >= FCGPU_MAX_PORTS || (nports && r.port >= nports)) {
            err = "route " + std::to_string(k) + ": bad OUTPUT";          // iproutetable.cc:111-113
            return FCGPU_EINVAL;
        }
        const uint32_t mask = r.plen ? 0xffffffffu << (32 - r.plen) : 0u;
        const auto key = std::make_pair(r.gw, (uint32_t)r.port);
        auto it = hop_of.find(key);
        if (it == hop_of.end()) {
            if (t.hops.size() > kLeafMax) { err = "more than 32767 next hops"; return FCGPU_EINVAL; }
            it = hop_of.emplace(key, (uint32_t)t.hops.size()).first;
            t.hops.push_back(NextHop{r.gw, r.port});
        }
        rs.push_back(R{host_order(r.addr) & mask, it->second, r.plen});   // addr &= mask, iproutetable.cc:41
        t.max_port = std::max(t.max_port, (uint32_t)r.port);
    }
    // ascending prefix length: a route's range then holds only shorter
    // prefixes' values when it is written, and it overwrites all of them
    std::stable_sort(rs.begin(), rs.end(), [](const R &a, const R &b) {
        return a.plen != b.plen ? a.plen < b.plen : a.addr < b.addr;
    });
    for (size_t k = 1; k < rs.size(); ++k)
        if (rs[k].plen == rs[k - 1].plen && rs[k].addr == rs[k - 1].addr) {
            const uint32_t a = rs[k].addr;
            err = "conflict with existing route '" + std::to_string(a >> 24) + "." + std::to_string((a >> 16) & 255) +
                  "." + std::to_string((a >> 8) & 255) + "." + std::to_string(a & 255) + "/" +
                  std::to_string(rs[k].plen) + "'";
            return FCGPU_EINVAL;
        }
    // the chunk below `e` (an entry of l0 or of a second-level chunk): a leaf
    // is split into a new chunk pre-filled with the leaf's value (leaf pushing)
    bool full = false;
    auto descend = [&](uint16_t &e) -> uint32_t {
        if (e & kChunkBit) return e & kLeafMax;
        const uint32_t c = t.nchunks();
        if (c >= kLeafMax) { full = true; return 0; }
        const uint16_t leaf = e;
        e = (uint16_t)(kChunkBit | c);            // before the resize: e may live in t.chunks
        t.chunks.resize(t.chunks.size() + 256, leaf);
        return c;
    };
    for (const R &r : rs) {
        const uint16_t hop = (uint16_t)r.hop;
        if (r.plen <= 16) {                       // controlled prefix expansion to /16
            std::fill_n(t.l0.begin() + (r.addr >> 16), 1u << (16 - r.plen), hop);
            continue;
        }
        uint32_t c = descend(t.l0[r.addr >> 16]);
        if (!full && r.plen <= 24) {              // ... to /24
            std::fill_n(t.chunks.begin() + c * 256 + ((r.addr >> 8) & 255), 1u << (24 - r.plen), hop);
            continue;
        }
        if (!full) {
            const size_t at = (size_t)c * 256 + ((r.addr >> 8) & 255);
            uint16_t e = t.chunks[at];
            c = descend(e);
            if (!full) {
                t.chunks[at] = e;
                std::fill_n(t.chunks.begin() + c * 256 + (r.addr & 255), 1u << (32 - r.plen), hop);   // ... to /32
            }
        }
        if (full) { err = "route table needs more than 32767 chunks"; return FCGPU_EINVAL; }
    }
    return FCGPU_OK;
}

// The walk, exactly as the device does it (fcgpu_device.hh route_walk): at
// most three dependent 2-byte loads, then the next hop. addr: raw network
// order. Returns the next-hop index (0 = no route).
inline uint32_t walk(const uint16_t *l0, const uint16_t *chunks, uint32_t addr) {
    const uint32_t a = host_order(addr);
    uint32_t e = l0[a >> 16];
    if (e & kChunkBit) {
        e = chunks[((e & kLeafMax) << 8) + ((a >> 8) & 255)];
        if (e & kChunkBit) e = chunks[((e & kLeafMax) << 8) + (a & 255)];
    }
    return e;
}

// IPRouteTable::lookup_route: the output port or -1; *gw (may be null) gets
// the route's gateway, 0 when it has none.
inline int lookup(const Table &t, uint32_t addr, uint32_t *gw) {
    const NextHop &h = t.hops[walk(t.l0.data(), t.chunks.data(), addr)];
    if (gw) *gw = h.port == kNoPort ? 0u : h.gw;
    return h.port == kNoPort ? -1 : (int)h.port;
}

// The device image: l0, the chunk pool, then the next hops (8 B each, padded
// to 16 B so a workgroup can stage them with whole uint4 loads). hop_off = the
// byte offset of the next hops.
inline std::vector<uint8_t> image(const Table &t, uint32_t &hop_off) {
    hop_off = (uint32_t)((t.l0.size() + t.chunks.size()) * sizeof(uint16_t));
    std::vector<uint8_t> img((hop_off + t.hops.size() * sizeof(NextHop) + 15u) & ~(size_t)15u, 0);
    std::copy_n(reinterpret_cast<const uint8_t *>(t.l0.data()), t.l0.size() * 2, img.begin());
    if (!t.chunks.empty())
        std::copy_n(reinterpret_cast<const uint8_t *>(t.chunks.data()), t.chunks.size() * 2, img.begin() + 131072);
    std::copy_n(reinterpret_cast<const uint8_t *>(t.hops.data()), t.hops.size() * sizeof(NextHop),
                img.begin() + hop_off);
    return img;
}

}  // namespace fcroute
