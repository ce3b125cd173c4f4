// fcgpu_espauth.hh -- k_espauth: IPsecAuthHMACSHA1 on the device
// (elements/ipsec/hmacsha1.cc:61-96 over hmac.cc:147-159, HMAC-SHA1-96 with
// a 16-byte key), a post-pass behind k_rx on the same stream. DESIGN.md 3.10.
//
// It reads the batch's verdicts, annotations and frames. A packet is
// considered iff its reason is FCGPU_R_OK, anno.ipver == 4 and the IP
// protocol byte is 50 (IPsecRouteTable::push case 0, ipsecroutetable.cc:
// 217-237). With e0 = nh + 4 * ihl, end = anno.length, elen = end - e0:
// SHORT if elen < 28, NO_SA if the SPI (big-endian word at e0) is not in the
// table; VERIFY hashes L = elen - 12 bytes from e0 and compares 12 digest
// bytes with the frame's last 12, COMPUTE hashes L = elen bytes, SEAL hashes
// as VERIFY and writes the 12 digest bytes to the frame's last 12 (the
// outbound IPsecAuthHMACSHA1(0) on a frame that holds the room). One 16-byte
// record per packet at the packet's own index; VERIFY and COMPUTE never
// write frames.
//
// SHA-1 over one message is a serial chain, so the parallelism is across
// packets: one lane per packet, 256 packets per tile, a workgroup looping
// over tiles. Per tile:
//   1. Setup: the lane reads verdict, annotation and descriptor, two header
//      dwords (ihl, protocol) and the SPI, finds its SA in the sorted image
//      (host/esp_sa.hh; in LDS up to 16 KB, else global) by a binary search
//      of uniform depth, and gets nb = (L + 9 + 63) / 64 blocks to compress.
//   2. Order (SORT): a counting sort of the tile by min(nb, 25) in LDS gives
//      every wave packets of similar length -- a wave runs until its longest
//      lane is done. Sorted slot j then carries packet s_pkt[j]; the record
//      goes to the packet's own index. A tile whose packets all have one
//      block count keeps its arrival order.
//   3. Per 64-byte step the wave fetches its 64 packets' next 64-byte
//      segments in the shape of k_rx's window gather: four LDS-DMA
//      instructions (global_load_lds_dwordx4), lane l of instruction k
//      fetching one 16-B chunk of packet 16k + l/4, so every four lanes read
//      one contiguous 64-B segment. Segments start at the 16-B aligned
//      address below arena + off + e0; rows are 64 B with the chunks
//      XOR-swizzled by row (k_rx's layout), so the lanes' ds_read_b128 are
//      conflict-free. Two 4-KB buffers per wave: while the 80 rounds of step
//      s run, segment s + 2 lands in the buffer segment s was read from
//      (block s needs segment s and the first chunk of s + 1).
//      No address passes the chunk that holds the packet's last byte
//      (clamped per packet, as ac_scan clamps alast): at most 15 B past the
//      frame's end, inside the ABI's 16-B slack.
//   4. Words: the lane holds 20 raw dwords; two levels of bit selects by a
//      mask take out the 17 at its dword misalignment and one v_perm_b32 per
//      word, with a
//      selector made from the byte misalignment, does the funnel shift and
//      the byte swap at once. No byte loads in the round loop.
//   5. Padding in registers: 0x80, the zeros and the bit length (64 + L) * 8
//      are merged by masks, only in the steps where some lane of the wave
//      holds its message's end (wave-uniform branch).
//   6. Rounds: 16 schedule registers updated in place, fully unrolled;
//      rotates are v_alignbit_b32, choose, majority and parity one
//      v_bitop3_b32 each (gfx950's three-input boolean, where gfx90a has
//      v_bfi_b32 / v_xor3_b32), the sums v_add3_u32.
//   7. The outer hash is one more compression from the outer midstate over
//      digest || 0x80 || 0.. || 672, in registers. VERIFY reads the packet's
//      last 12 bytes from the arena as four aligned dwords, issued before the
//      outer rounds. One 16-byte record store per lane.
//   8. Statistics: per-status wave counts by ballot, kept over the
//      workgroup's tiles; one atomic per non-zero counter per workgroup.
// LDS per workgroup: 4 x 8 KB segment buffers + 4 KB packet slots + 160 B,
// and the SA image (<= 16 KB, dynamic): three workgroups per CU with the
// image, four without.
#pragma once
#include "fcgpu_device.hh"

namespace fcgpu {

constexpr uint32_t kEspLdsImage = 16384;        // SA images up to this size are staged in LDS
constexpr uint32_t kEspSaWords = 12;            // {spi, inner[5], outer[5], 0}
constexpr uint32_t kEspBins = 26;               // nb 0 (nothing to hash) .. 25 (and more)
constexpr uint32_t kEspStatWords = 8;           // ok, bad, no_sa, too_short, not_esp

struct EspArgs {
    const uint8_t *arena;
    const uint2 *desc;
    const uint16_t *verdict;      // [n] k_rx's verdicts
    const uint32_t *anno;         // [n] fcgpu_anno as 4 words each
    uint32_t n, ntiles;
    uint32_t mode;                // FCGPU_ESP_VERIFY / FCGPU_ESP_COMPUTE / FCGPU_ESP_SEAL (which writes the arena)
    const uint32_t *sa;           // [nsa * kEspSaWords], sorted by spi
    uint32_t nsa;                 // >= 1
    uint32_t sa_lds;              // the image is staged in (dynamic) LDS
    uint4 *rec;                   // [n] records
    unsigned long long *stat;     // [kEspStatWords]
};

// One packet's slot after setup (16 B in LDS):
//   x  arena offset of the frame, rounded down to 16
//   y  rb | lastc << 17: rb = (off & 15) + e0, the first message byte
//      relative to x; lastc = the last 16-B chunk (relative to x) that may be
//      read
//   z  L | status << 16 | lane << 24 (the packet's lane in the tile)
//   w  index of its SA
struct __attribute__((aligned(16))) EspSlot {
    uint32_t x, y, z, w;
};

__device__ __forceinline__ uint32_t esp_rol(uint32_t v, uint32_t r) { return __builtin_amdgcn_alignbit(v, v, 32u - r); }

// FIPS 180-1 section 7, method 2: an in-place 16-word schedule.
#define FCGPU_SHA1_W(t) \
    (w[(t) & 15] = esp_rol(w[((t) + 13) & 15] ^ w[((t) + 8) & 15] ^ w[((t) + 2) & 15] ^ w[(t) & 15], 1))
#define FCGPU_SHA1_STEP(f, k, wt)                    \
    {                                                \
        const uint32_t tmp = esp_rol(a, 5) + (f) + e + (k) + (wt); \
        e = d;                                       \
        d = c;                                       \
        c = esp_rol(b, 30);                          \
        b = a;                                       \
        a = tmp;                                     \
    }
// h += compress(h, w); w is used up. Lanes with act false keep h.
__device__ __forceinline__ void sha1_block(uint32_t (&h)[5], uint32_t (&w)[16], bool act) {
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
#pragma unroll
    for (int t = 0; t < 16; ++t) FCGPU_SHA1_STEP(d ^ (b & (c ^ d)), 0x5A827999u, w[t])
#pragma unroll
    for (int t = 16; t < 20; ++t) FCGPU_SHA1_STEP(d ^ (b & (c ^ d)), 0x5A827999u, FCGPU_SHA1_W(t))
#pragma unroll
    for (int t = 20; t < 40; ++t) FCGPU_SHA1_STEP(b ^ c ^ d, 0x6ED9EBA1u, FCGPU_SHA1_W(t))
#pragma unroll
    for (int t = 40; t < 60; ++t) FCGPU_SHA1_STEP(c ^ ((b ^ c) & (d ^ c)), 0x8F1BBCDCu, FCGPU_SHA1_W(t))
#pragma unroll
    for (int t = 60; t < 80; ++t) FCGPU_SHA1_STEP(b ^ c ^ d, 0xCA62C1D6u, FCGPU_SHA1_W(t))
    h[0] = act ? h[0] + a : h[0];
    h[1] = act ? h[1] + b : h[1];
    h[2] = act ? h[2] + c : h[2];
    h[3] = act ? h[3] + d : h[3];
    h[4] = act ? h[4] + e : h[4];
}
#undef FCGPU_SHA1_STEP
#undef FCGPU_SHA1_W

// SEAL: the 12 digest bytes (three little-endian words) to arena + at,
// whatever its alignment, by naturally aligned stores of own bytes only: a
// head of 0-3 bytes (byte / short), two or three dwords, a tail.
__device__ __forceinline__ void esp_store12(uint8_t *arena, size_t at, uint32_t w0, uint32_t w1, uint32_t w2) {
    uint8_t *p = arena + at;
    const uint32_t m = (uint32_t)at & 3u;
    if (m == 0) {
        uint32_t *q = reinterpret_cast<uint32_t *>(p);
        q[0] = w0;
        q[1] = w1;
        q[2] = w2;
        return;
    }
    // head: 4 - m bytes
    if (m & 1u) *p = (uint8_t)w0;
    if (m == 1u) *reinterpret_cast<uint16_t *>(p + 1) = (uint16_t)(w0 >> 8);
    if (m == 2u) *reinterpret_cast<uint16_t *>(p) = (uint16_t)w0;
    uint32_t *q = reinterpret_cast<uint32_t *>(p + 4 - m);
    q[0] = __builtin_amdgcn_alignbyte(w1, w0, 4u - m);
    q[1] = __builtin_amdgcn_alignbyte(w2, w1, 4u - m);
    // tail: m bytes, the top of w2
    uint8_t *e = p + 12 - m;
    if (m == 1u) *e = (uint8_t)(w2 >> 24);
    if (m == 2u) *reinterpret_cast<uint16_t *>(e) = (uint16_t)(w2 >> 16);
    if (m == 3u) {
        *reinterpret_cast<uint16_t *>(e) = (uint16_t)(w2 >> 8);
        e[2] = (uint8_t)(w2 >> 24);
    }
}

// The wave's gather of segment `seg` (64 B per packet) into buf (4 KB): lane l
// of instruction k fetches chunk (l & 3) ^ swizzle of slot wbase + 16k + l/4,
// clamped to the slot's last readable chunk.
__device__ __forceinline__ void esp_fetch(const uint8_t *arena, const EspSlot *s_pkt, uint32_t wbase, uint32_t lane,
                                          uint32_t seg, uint8_t *buf) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t p = k * 16 + (lane >> 2);
        const uint2 P = *reinterpret_cast<const uint2 *>(&s_pkt[wbase + p]);
        const uint32_t c = (lane & 3) ^ ((p >> 2) & 3);
        const uint32_t want = ((P.y & 0x1ffffu) >> 4) + 4 * seg + c, lastc = P.y >> 17;
        const uint32_t ci = want < lastc ? want : lastc;
        glds16(arena + P.x + (size_t)ci * 16, buf + k * 1024);
    }
}

template <bool SORT>
__global__ __launch_bounds__(kTile) void k_espauth(const EspArgs A) {
    extern __shared__ uint4 s_sa[];                          // the SA image (A.sa_lds)
    __shared__ __attribute__((aligned(16))) uint8_t s_seg[kTile / kWave][2][kWave * 64];
    __shared__ EspSlot s_pkt[kTile];
    __shared__ uint32_t s_bin[32];
    __shared__ uint32_t s_tot[kEspStatWords];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wbase = wave * kWave;
    if (A.sa_lds)
        for (uint32_t q = tid; q < A.nsa * 3; q += kTile) s_sa[q] = reinterpret_cast<const uint4 *>(A.sa)[q];
    if (tid < kEspStatWords) s_tot[tid] = 0;
    const uint32_t *lsa = reinterpret_cast<const uint32_t *>(s_sa);
    auto sa_word = [&](uint32_t idx, uint32_t k) -> uint32_t {   // two branches, not a pointer select (flat loads)
        if (A.sa_lds) return lsa[idx * kEspSaWords + k];
        return A.sa[(size_t)idx * kEspSaWords + k];
    };
    uint32_t cnt[5] = {0, 0, 0, 0, 0};                         // wave-uniform: packets per status
    uint8_t *const buf0 = s_seg[wave][0], *const buf1 = s_seg[wave][1];
    const uint32_t sw = (lane >> 2) & 3;
    for (uint32_t tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
        __syncthreads();                                       // the image is staged; the last tile's slots are read
        // ---- 1. setup ---------------------------------------------------
        const uint32_t i = tile * kTile + tid;
        const bool live = i < A.n;
        const uint32_t ic = live ? i : A.n - 1;                // a lane past the batch gets a readable address
        const uint2 d = A.desc[ic];
        const uint32_t v = A.verdict[ic];
        const uint32_t an1 = A.anno[4 * (size_t)ic + 1], an2 = A.anno[4 * (size_t)ic + 2], an3 = A.anno[4 * (size_t)ic + 3];
        const uint32_t end = an1 & 0xffffu, nh = an2 & 0xffffu, ipver = (an3 >> 8) & 0xffu;
        uint32_t status = FCGPU_ESP_NOT_ESP, L = 0, e0 = 0, said = 0;
        const bool ip4 = live && (v & 0xffu) == FCGPU_R_OK && ipver == 4;
        // aligned dword holding arena byte o (the arena is 16-B aligned, as k_rx's windows assume)
        auto adw = [&](size_t o) -> const uint32_t * { return reinterpret_cast<const uint32_t *>(A.arena + (o & ~(size_t)3)); };
        if (ip4) {
            // header bytes 0 (ihl) and 9 (protocol): aligned dwords inside the frame
            const size_t o0 = (size_t)d.x + nh, o9 = o0 + 9;
            const uint32_t ihl = (*adw(o0) >> (8 * (o0 & 3))) & 15u;
            const uint32_t proto = (*adw(o9) >> (8 * (o9 & 3))) & 0xffu;
            e0 = nh + 4 * ihl;
            if (proto == 50) {
                const int elen = (int)end - (int)e0;
                if (elen < 28) {
                    status = FCGPU_ESP_SHORT;
                } else {
                    // the SPI: the big-endian word at e0 (inside the frame: elen >= 28)
                    const size_t os = (size_t)d.x + e0;
                    const uint32_t *pa = adw(os);
                    const uint32_t spi = __builtin_bswap32(__builtin_amdgcn_alignbyte(pa[1], pa[0], (uint32_t)(os & 3)));
                    uint32_t lo = 0;
                    for (uint32_t len = A.nsa; len > 1;) {     // uniform depth
                        const uint32_t half = len >> 1;
                        if (sa_word(lo + half, 0) <= spi) lo += half;
                        len -= half;
                    }
                    if (sa_word(lo, 0) == spi) {
                        status = FCGPU_ESP_OK;                 // VERIFY decides OK / BAD at the end
                        said = lo;
                        L = A.mode == FCGPU_ESP_COMPUTE ? (uint32_t)elen : (uint32_t)elen - 12u;
                    } else {
                        status = FCGPU_ESP_NO_SA;
                    }
                }
            }
        }
        const bool hashed = status == FCGPU_ESP_OK;
        const uint32_t nb = hashed ? (L + 9 + 63) >> 6 : 0u;
        EspSlot S;
        S.x = d.x & ~15u;
        const uint32_t rbs = hashed ? (d.x & 15u) + e0 : (d.x & 15u);
        // the last chunk read: the one holding the packet's last byte (a packet that is not hashed: its first)
        const uint32_t lastc = hashed ? ((d.x & 15u) + end - 1) >> 4 : 0u;
        S.y = rbs | lastc << 17;
        S.z = L | status << 16 | tid << 24;
        S.w = said;
        // ---- 2. order by nb -----------------------------------------------
        uint32_t pos = tid;
        if (SORT) {
            const uint32_t bin = nb < kEspBins - 1 ? nb : kEspBins - 1;
            if (tid < 32) s_bin[tid] = tid == 31 ? nb : 0u;     // word 31: one lane's nb, no bin
            __syncthreads();
            // a tile of one block count keeps its order: 256 atomics on one bin
            // cost a 64-B batch 5 % (block-uniform: the barrier below is safe)
            if (!__syncthreads_and(nb == s_bin[31])) {
                const uint32_t rank = atomicAdd(&s_bin[bin], 1u);
                __syncthreads();
                uint32_t base = 0;                             // packets in the bins above mine: longest first
                for (uint32_t b = kEspBins - 1; b > bin; --b) base += s_bin[b];
                pos = base + rank;
            }
        }
        s_pkt[pos] = S;
        __syncthreads();
        const EspSlot M = s_pkt[tid];                          // this lane's packet
        const uint32_t mL = M.z & 0xffffu, mstatus = (M.z >> 16) & 0xffu, mlane = M.z >> 24;
        const bool mhashed = mstatus == FCGPU_ESP_OK;
        const uint32_t mnb = mhashed ? (mL + 9 + 63) >> 6 : 0u;
        const uint32_t rb = M.y & 0x1ffffu, r = rb & 15u;
        uint32_t maxnb = mnb;
#pragma unroll
        for (int o = 32; o; o >>= 1) {
            const uint32_t x = __shfl_xor(maxnb, o);
            maxnb = x > maxnb ? x : maxnb;
        }
        uint32_t h[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) h[k] = sa_word(M.w, 1 + k);      // the inner midstate (slot 0's for idle lanes)
        // ---- 3..6. the message blocks -------------------------------------
        if (maxnb) {                                                 // wave-uniform
            esp_fetch(A.arena, s_pkt, wbase, lane, 0, buf0);
            esp_fetch(A.arena, s_pkt, wbase, lane, 1, buf1);
            const uint32_t sel = 0x00010203u + (r & 3u) * 0x01010101u;   // v_perm: big-endian word at byte r & 3 of {hi, lo}
            const uint32_t q1 = 0u - ((r >> 2) & 1u), q2 = 0u - ((r >> 3) & 1u);   // all ones: skip one / two dwords
            for (uint32_t s = 0; s < maxnb; ++s) {
                uint8_t *cur = (s & 1) ? buf1 : buf0, *nxt = (s & 1) ? buf0 : buf1;
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // segments s and s + 1 have landed
                __builtin_amdgcn_wave_barrier();
                uint32_t raw[20];
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const uint4 q = *reinterpret_cast<const uint4 *>(cur + lane * 64 + ((c ^ sw) << 4));
                    raw[4 * c] = q.x; raw[4 * c + 1] = q.y; raw[4 * c + 2] = q.z; raw[4 * c + 3] = q.w;
                }
                {
                    const uint4 q = *reinterpret_cast<const uint4 *>(nxt + lane * 64 + (sw << 4));
                    raw[16] = q.x; raw[17] = q.y; raw[18] = q.z; raw[19] = q.w;
                }
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // every lane has its rows: cur may be overwritten
                __builtin_amdgcn_wave_barrier();
                if (s + 2 <= maxnb) esp_fetch(A.arena, s_pkt, wbase, lane, s + 2, cur);
                // the 17 dwords from dword r / 4 on, then one permute per word
                // (bit selects by a mask: `q ? raw[k + 2] : raw[k]` became an
                // array in scratch indexed by q)
                uint32_t t2[18], t1[17], w[16];
#pragma unroll
                for (int k = 0; k < 18; ++k) t2[k] = (raw[k + 2] & q2) | (raw[k] & ~q2);
#pragma unroll
                for (int k = 0; k < 17; ++k) t1[k] = (t2[k + 1] & q1) | (t2[k] & ~q1);
#pragma unroll
                for (int k = 0; k < 16; ++k) w[k] = __builtin_amdgcn_perm(t1[k + 1], t1[k], sel);
                const bool act = s < mnb;
                const uint32_t p0 = 64 * s;
                if (__ballot(act && p0 + 64 > mL)) {                  // some lane's message ends here: pad by masks
#pragma unroll
                    for (int k = 0; k < 16; ++k) {
                        const int rem = (int)mL - (int)(p0 + 4 * k);  // message bytes from this word on
                        const uint32_t sh = 8u * (uint32_t)(rem & 3);
                        const uint32_t part = (w[k] & ~(0xffffffffu >> sh)) | (0x80000000u >> sh);
                        w[k] = rem >= 4 ? w[k] : rem < 0 ? 0u : part;
                    }
                    if (s + 1 == mnb) w[15] = (64u + mL) * 8u;        // word 14 is 0: L < 2^16
                }
                sha1_block(h, w, act);
            }
        }
        // ---- 7. the outer hash, the verdict, the record -------------------
        uint32_t got[4] = {0, 0, 0, 0};
        uint32_t gsh = 0;
        const bool verify = mhashed && A.mode == FCGPU_ESP_VERIFY;
        if (verify) {   // frame[end - 12, end): four aligned dwords, the last at most 3 B past the end
            const size_t oi = (size_t)M.x + rb + mL;
            const uint32_t *pa = reinterpret_cast<const uint32_t *>(A.arena + (oi & ~(size_t)3));
            gsh = (uint32_t)(oi & 3);
#pragma unroll
            for (int k = 0; k < 4; ++k) got[k] = pa[k];
        }
        uint32_t ho[5], w[16];
#pragma unroll
        for (int k = 0; k < 5; ++k) ho[k] = sa_word(M.w, 6 + k);
#pragma unroll
        for (int k = 0; k < 5; ++k) w[k] = h[k];
        w[5] = 0x80000000u;
#pragma unroll
        for (int k = 6; k < 15; ++k) w[k] = 0;
        w[15] = (64u + 20u) * 8u;
        if (__ballot(mhashed)) sha1_block(ho, w, true);
        uint32_t st = mstatus;
        const uint32_t i0 = __builtin_bswap32(ho[0]), i1 = __builtin_bswap32(ho[1]), i2 = __builtin_bswap32(ho[2]);
        if (verify) {
            const bool same = __builtin_amdgcn_alignbyte(got[1], got[0], gsh) == i0 &&
                              __builtin_amdgcn_alignbyte(got[2], got[1], gsh) == i1 &&
                              __builtin_amdgcn_alignbyte(got[3], got[2], gsh) == i2;
            st = same ? FCGPU_ESP_OK : FCGPU_ESP_BAD;
        }
        const uint32_t oi = tile * kTile + mlane;
        if (oi < A.n) A.rec[oi] = mhashed ? make_uint4(st, i0, i1, i2) : make_uint4(st, 0u, 0u, 0u);
        if (mhashed && A.mode == FCGPU_ESP_SEAL)   // frame[end - 12, end): where VERIFY reads
            esp_store12(const_cast<uint8_t *>(A.arena), (size_t)M.x + rb + mL, i0, i1, i2);
        // ---- 8. statistics -------------------------------------------------
        const bool mlive = oi < A.n;
        cnt[0] += (uint32_t)__popcll(__ballot(mlive && st == FCGPU_ESP_OK));
        cnt[1] += (uint32_t)__popcll(__ballot(mlive && st == FCGPU_ESP_BAD));
        cnt[2] += (uint32_t)__popcll(__ballot(mlive && st == FCGPU_ESP_NO_SA));
        cnt[3] += (uint32_t)__popcll(__ballot(mlive && st == FCGPU_ESP_SHORT));
        cnt[4] += (uint32_t)__popcll(__ballot(mlive && st == FCGPU_ESP_NOT_ESP));
    }
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (cnt[k]) atomicAdd(&s_tot[k], cnt[k]);
    __syncthreads();
    if (tid < 5 && s_tot[tid]) atomicAdd(A.stat + tid, (unsigned long long)s_tot[tid]);
}

}  // namespace fcgpu
