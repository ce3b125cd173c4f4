// fcgpu_match.hh -- k_acmatch, the payload pre-pass of FCGPU_CLS_STRING: every
// frame of a batch is run through the Aho-Corasick automaton of
// host/ac_table.hh and its earliest match is left in one uint32 record per
// packet, which the ROUTE == 3 instances of k_rx turn into the port
// (fcgpu_device.hh match_apply). DESIGN.md 3.8.
//
// Record: 0 = no match anywhere in the frame, else end << 16 | (1 + id) for
// the match with the earliest end position (1..65535) over the whole frame,
// the longest pattern of those ending there. k_rx accepts it iff end <=
// anno.length: if the earliest match of the untrimmed frame ends past the
// trim, none ends inside it, so the pre-pass needs no verdict.
//
// Work split: 16 lanes per packet, four packets per wave (wave_l4_sum's
// split). The group copies its frame into LDS with coalesced 16-byte loads
// (the arena is readable 16 B past a frame's end), then lane j scans chunks
// j, j + 16, ... of S bytes: chunk k starts in the root state at byte k * S
// and runs to min(len, (k + 1) * S + Lmax - 1), stopping at its first final
// state. Every candidate is a real match, so the least end position over the
// lanes is the earliest one; of the chunks that report it the lowest started
// at least Lmax bytes before it (the chunk below does not reach it), so it
// has seen every pattern ending there and its id is the longest. The group
// takes the minimum of (end, k) with four lane exchanges.
//
// Per text byte the dependent chain is one read, state = next[state *
// classes + class]; a state is final iff state >= first_final (the builder
// numbers final states last), so no second table is read until a lane stops.
// The classes of a lane's next dword are looked up while the chain of the
// current one runs.
#pragma once
#include "fcgpu_device.hh"

namespace fcgpu {

constexpr uint32_t kAcLanes = 16;                      // lanes per packet
constexpr uint32_t kAcGroups = kTile / kAcLanes;       // packets a workgroup scans at a time
constexpr uint32_t kAcTextCap = 1536;                  // frame bytes (alignment shift included) staged in LDS
constexpr uint32_t kAcTextBuf = kAcTextCap + 32;       // ... and room for the dword read ahead
// Class map + next[] sit in LDS up to this size; with the text buffers a
// workgroup then stays below 64 KB, two to a CU's 160 KB.
constexpr uint32_t kAcLdsTable = 36u * 1024u;
constexpr uint32_t kAcChunkMin = 32;                   // S >= 32: chunk numbers fit 11 bits for 65535-B frames

struct AcArgs {
    const uint8_t *arena;
    const uint2 *desc;
    uint32_t n;
    uint32_t layout;          // kLay* bits of the descriptors
    uint32_t *rec;            // [n] records
    const uint8_t *image;     // host/ac_table.hh: class map, next at byte 256, out at out_off
    uint32_t out_off;
    uint32_t nclasses;
    uint32_t first_final;
    uint32_t lmax;
    uint32_t chunk;           // S
    uint32_t table_q;         // uint4 words staged in LDS: the class map (16), with next[] when it fits
};

__host__ __device__ inline bool ac_next_in_lds(uint32_t out_off) { return out_off <= kAcLdsTable; }
__host__ __device__ inline uint32_t ac_chunk(uint32_t lmax) {
    uint32_t s = kAcChunkMin;
    while (s < lmax) s <<= 1;     // the overlap Lmax - 1 never more than doubles the bytes scanned
    return s;
}
inline size_t ac_lds_bytes(const AcArgs &a) { return (size_t)a.table_q * 16 + (size_t)kAcGroups * kAcTextBuf; }

// One chunk: text bytes [p0, e) from the root. The text is the group's LDS
// copy (TXT_LDS; byte p at txt[shift + p]) or, for a frame too long for it,
// the arena (g = the frame's 16-B aligned base). Returns the end position of
// the first final state (0: none) and that state.
template <bool TAB_LDS, bool TXT_LDS>
__device__ __forceinline__ uint32_t ac_scan(const AcArgs &A, const uint8_t *s_cls, const uint16_t *s_next,
                                            const uint8_t *txt, const uint8_t *g, uint32_t shift, uint32_t p0,
                                            uint32_t e, uint32_t &fstate) {
    const uint16_t *gnext = reinterpret_cast<const uint16_t *>(A.image + 256);
    const uint32_t x0 = shift + p0, x1 = shift + e, span = x1 - x0;
    const uint32_t alast = (x1 - 1) & ~3u;      // the last dword holding text: nothing is read past it
    const uint32_t ncls = A.nclasses, ff = A.first_final;
    auto text = [&](uint32_t a) -> uint32_t {
        return TXT_LDS ? *reinterpret_cast<const uint32_t *>(txt + a) : *reinterpret_cast<const uint32_t *>(g + a);
    };
    uint32_t a = x0 & ~3u;
    uint32_t w = text(a);
    uint32_t c[4], nc[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) c[b] = s_cls[(w >> (8 * b)) & 255u];
    uint32_t st = 0, found = 0;
    for (; a < x1; a += 4) {
        // the next dword's classes: off the state chain
        w = text(a + 4 <= alast ? a + 4 : alast);
#pragma unroll
        for (int b = 0; b < 4; ++b) nc[b] = s_cls[(w >> (8 * b)) & 255u];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t x = a + b;
            const bool in = x - x0 < span && !found;      // bytes of the first and last dword outside [x0, x1)
            const uint32_t t = TAB_LDS ? s_next[st * ncls + c[b]] : gnext[st * ncls + c[b]];
            st = in ? t : st;
            if (in && t >= ff) found = x + 1 - shift;
        }
        if (found) break;
#pragma unroll
        for (int b = 0; b < 4; ++b) c[b] = nc[b];
    }
    fstate = st;
    return found;
}

// Grid: a few workgroups per CU, each looping over 16-packet steps, so the
// table is staged once per workgroup.
template <bool TAB_LDS>
__global__ __launch_bounds__(kTile) void k_acmatch(AcArgs A) {
    extern __shared__ uint4 s_ac[];
    const uint4 *img = reinterpret_cast<const uint4 *>(A.image);
    for (uint32_t q = threadIdx.x; q < A.table_q; q += kTile) s_ac[q] = img[q];
    __syncthreads();
    const uint8_t *s_cls = reinterpret_cast<const uint8_t *>(s_ac);
    const uint16_t *s_next = reinterpret_cast<const uint16_t *>(s_cls + 256);
    const uint32_t grp = threadIdx.x / kAcLanes, j = threadIdx.x % kAcLanes;
    uint8_t *txt = reinterpret_cast<uint8_t *>(s_ac + A.table_q) + grp * kAcTextBuf;
    const uint32_t S = A.chunk, steps = (A.n + kAcGroups - 1) / kAcGroups;
    for (uint32_t step = blockIdx.x; step < steps; step += gridDim.x) {
        const uint32_t i = step * kAcGroups + grp;
        uint2 d = make_uint2(0, 0);
        if (i < A.n) d = load_desc(A.desc, i, A.layout);
        const uint32_t len = d.y < 65535u ? d.y : 65535u;     // a later end would not fit anno.length either
        const uint32_t shift = d.x & 15u, hi = shift + len;
        const uint8_t *g = A.arena + (d.x & ~15u);
        const bool in_lds = hi <= kAcTextCap;                 // group-uniform
        // the previous step's scans are done before the buffer is overwritten
        __builtin_amdgcn_wave_barrier();
        if (in_lds)
            for (uint32_t o = 16 * j; o < hi; o += 16 * kAcLanes)
                *reinterpret_cast<uint4 *>(txt + o) = *reinterpret_cast<const uint4 *>(g + o);
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
        // lane j: chunks j, j + 16, ... in order; its first match is its
        // earliest (a later chunk sees a subset of the matches)
        uint32_t key = 0xffffffffu, id1 = 0;
        for (uint32_t k = j; k * S < len; k += kAcLanes) {
            const uint32_t p0 = k * S, e = p0 + S + A.lmax - 1 < len ? p0 + S + A.lmax - 1 : len;
            uint32_t fs = 0;
            const uint32_t end = in_lds ? ac_scan<TAB_LDS, true>(A, s_cls, s_next, txt, g, shift, p0, e, fs)
                                        : ac_scan<TAB_LDS, false>(A, s_cls, s_next, txt, g, shift, p0, e, fs);
            if (end) {
                key = end << 11 | k;      // k <= 65535 / 32
                id1 = reinterpret_cast<const uint16_t *>(A.image + A.out_off)[fs - A.first_final];
                break;
            }
        }
        uint32_t kmin = key;
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) {
            const uint32_t x = __shfl_xor(kmin, o);
            kmin = x < kmin ? x : kmin;
        }
        // the one lane that holds the minimum hands over its id
        const uint64_t own = __ballot(key == kmin && key != 0xffffffffu);
        const uint32_t mine = (uint32_t)(own >> (threadIdx.x & 48u)) & 0xffffu;
        const uint32_t src = (threadIdx.x & 48u) + (mine ? (uint32_t)__builtin_ctz(mine) : 0u);
        const uint32_t id = __shfl(id1, (int)src);
        if (j == 0 && i < A.n) A.rec[i] = mine ? (kmin >> 11) << 16 | id : 0u;
    }
}

}  // namespace fcgpu
