// fcgpu_espaes.hh -- k_espaes: IPsecAES(0) on the device (elements/ipsec/
// aes.cc:69-138, decrypt branch: AES-128 in the element's 8-byte-IV chaining),
// a post-pass behind k_rx and in front of k_espauth on the same stream,
// decrypting in place in the arena. Semantics: include/fastclick_gpu.h;
// DESIGN.md 3.11.
//
// Unlike SHA-1 the work is parallel inside a packet: block i needs only its
// own 16 ciphertext bytes and the first 8 of block i - 1 (or the IV). A
// 1500-byte frame has 91 blocks, a 64-byte one at most 1, so the unit of work
// is the block. Per tile of `tpk` packets (256, fewer when the batch has too
// few packets to fill the device) a workgroup of 256 lanes does:
//   1. Setup, one lane per packet as in k_espauth: status, the SA by a binary
//      search of uniform depth (image in LDS up to 16 KB, else global), nblk.
//      The status byte goes to the packet's own index.
//   2. An exclusive prefix sum of nblk over the tile in LDS (wave scans by
//      shuffles, then the four wave totals).
//   3. Passes over the tile's flattened block list, 256 blocks each: lane t of
//      pass p takes block g = 256 p + t, finds its packet j by a binary search
//      of the prefix array (the last j with pre[j] <= g), i = g - pre[j].
//   4. Inputs: 5 aligned dwords over the block and 3 over its chain bytes (the
//      IV for i = 0, else C_{i-1}[0, 8)), funnel-shifted by v_alignbyte_b32.
//   5. Ordering. In place, block i's lane overwrites what block i + 1's lane
//      reads. The loop is software-pipelined:
//          load(pass 0); for p: load(p + 1); compute(p); wait; barrier; store(p)
//      so every byte a lane of the workgroup needs of passes <= p + 1 is in a
//      register before any lane stores pass p. Pass p + 2's loads come after
//      that barrier and race with the stores of pass p, but they need only
//      bytes of passes p + 1 and p + 2 and IVs, which pass p does not write.
//      A workgroup owns whole packets, so no chain crosses workgroups.
//   6. The block: the equivalent inverse cipher (FIPS 197 5.3.5) on
//      little-endian columns, 9 rounds of 16 lookups in Td0 and its three
//      rotations, the last round 16 lookups in the inverse S-box. Tables in
//      LDS: NTAB = 4 keeps the four rotations, NTAB = 1 rotates one table by
//      v_alignbit_b32; REPL interleaved replicas (word x of replica r at
//      x * REPL + r, lane l uses r = l % REPL) spread the 64 lanes' random
//      lookups over more banks. Round keys: 44 words of the lane's SA, LDS or
//      global by two plain branches; lanes of one SA read them as broadcasts.
//   7. Stores write the block's own 16 bytes and no other: by the address's
//      low two bits a head of 0-3 bytes (byte / short stores), three or four
//      aligned dwords, a tail. No read-modify-write of a shared word.
//   8. Statistics by ballot, one atomic per non-zero counter per workgroup.
#pragma once
#include "fcgpu_device.hh"
#include "host/aes_key.hh"

namespace fcgpu {

constexpr uint32_t kAesLdsImage = 16384;        // SA images up to this size (85 SAs) are staged in LDS
constexpr uint32_t kAesSaWords = 48;            // {spi, rk[44], pad[3]}
constexpr uint32_t kAesStatWords = 6;           // ok, no_sa, too_short, unaligned, not_esp, blocks
constexpr uint32_t kAesDefaultTables = 1;       // the measured choice
constexpr uint32_t kAesDefaultReplicas = 1;

struct AesArgs {
    uint8_t *arena;
    const uint2 *desc;
    const uint16_t *verdict;      // [n] k_rx's verdicts
    const uint32_t *anno;         // [n] fcgpu_anno as 4 words each
    uint32_t n, ntiles;
    uint32_t tpk;                 // packets per tile: a power of two <= kTile
    const uint32_t *sa;           // [nsa * kAesSaWords], sorted by spi
    uint32_t nsa;                 // >= 1
    uint32_t sa_lds;              // the image is staged in (dynamic) LDS
    const uint32_t *td0;          // [256] Td0
    const uint32_t *isb;          // [64] the inverse S-box, four bytes a word
    uint8_t *status;              // [n]
    unsigned long long *stat;     // [kAesStatWords]
};

// One block's inputs in registers.
struct AesIn {
    uint32_t c[4];                // the ciphertext block
    uint32_t x[2];                // what its first 8 bytes are XORed with
    size_t at;                    // arena offset of the block
    uint32_t said;
    bool act;
};

template <int NTAB, int REPL, bool SA_LDS>
__device__ __forceinline__ void aes_block(const AesIn &I, const uint32_t *s_td, const uint8_t *s_isb, const uint32_t *lsa,
                                          const uint32_t *gsa, uint32_t rep, uint32_t (&o)[4]) {
    const uint32_t *rk = (SA_LDS ? lsa : gsa) + (size_t)I.said * kAesSaWords + 1;
    auto T = [&](int t, uint32_t x) -> uint32_t {
        if (NTAB == 4) return s_td[t * 256 * REPL + x * REPL + rep];
        const uint32_t v = s_td[x * REPL + rep];
        return t ? __builtin_amdgcn_alignbit(v, v, 32u - 8u * t) : v;
    };
    auto S = [&](uint32_t x) -> uint32_t { return s_isb[x * REPL + rep]; };
    uint32_t s[4], t[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) s[c] = I.c[c] ^ rk[c];
#pragma unroll
    for (int r = 1; r < 10; ++r) {
#pragma unroll
        for (int c = 0; c < 4; ++c)
            t[c] = T(0, s[c] & 0xffu) ^ T(1, (s[(c + 3) & 3] >> 8) & 0xffu) ^ T(2, (s[(c + 2) & 3] >> 16) & 0xffu) ^
                   T(3, s[(c + 1) & 3] >> 24) ^ rk[4 * r + c];
#pragma unroll
        for (int c = 0; c < 4; ++c) s[c] = t[c];
    }
#pragma unroll
    for (int c = 0; c < 4; ++c)
        o[c] = (S(s[c] & 0xffu) | S((s[(c + 3) & 3] >> 8) & 0xffu) << 8 | S((s[(c + 2) & 3] >> 16) & 0xffu) << 16 |
                S(s[(c + 1) & 3] >> 24) << 24) ^ rk[40 + c];
    o[0] ^= I.x[0];
    o[1] ^= I.x[1];
}

// The block's own 16 bytes to arena + at, whatever its alignment, by naturally
// aligned stores.
__device__ __forceinline__ void aes_store(uint8_t *arena, size_t at, const uint32_t (&o)[4]) {
    uint8_t *p = arena + at;
    const uint32_t m = (uint32_t)at & 3u;
    if (m == 0) {
        if (((uint32_t)at & 15u) == 0) {
            *reinterpret_cast<uint4 *>(p) = make_uint4(o[0], o[1], o[2], o[3]);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) reinterpret_cast<uint32_t *>(p)[k] = o[k];
        }
        return;
    }
    // head: 4 - m bytes
    if (m & 1u) *p = (uint8_t)o[0];
    if (m == 1u) *reinterpret_cast<uint16_t *>(p + 1) = (uint16_t)(o[0] >> 8);
    if (m == 2u) *reinterpret_cast<uint16_t *>(p) = (uint16_t)o[0];
    uint32_t *q = reinterpret_cast<uint32_t *>(p + 4 - m);
#pragma unroll
    for (int k = 0; k < 3; ++k) q[k] = __builtin_amdgcn_alignbyte(o[k + 1], o[k], 4u - m);
    // tail: m bytes, the top of o[3]
    uint8_t *e = p + 16 - m;
    if (m == 1u) *e = (uint8_t)(o[3] >> 24);
    if (m == 2u) *reinterpret_cast<uint16_t *>(e) = (uint16_t)(o[3] >> 16);
    if (m == 3u) {
        *reinterpret_cast<uint16_t *>(e) = (uint16_t)(o[3] >> 8);
        e[2] = (uint8_t)(o[3] >> 24);
    }
}

template <int NTAB, int REPL>
__global__ __launch_bounds__(kTile) void k_espaes(const AesArgs A) {
    extern __shared__ uint4 s_dyn[];                           // the SA image (A.sa_lds)
    __shared__ uint32_t s_td[NTAB * 256 * REPL];
    __shared__ __attribute__((aligned(4))) uint8_t s_isb[256 * REPL];
    __shared__ uint32_t s_pre[kTile + 1];                      // exclusive prefix of nblk
    __shared__ uint32_t s_off[kTile];                          // frame offset
    __shared__ uint32_t s_sae[kTile];                          // e0 + 16 | SA index << 16
    __shared__ uint32_t s_wsum[kTile / kWave];
    __shared__ uint32_t s_tot[kAesStatWords];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t rep = lane & (REPL - 1);
    if (A.sa_lds)
        for (uint32_t q = tid; q < A.nsa * (kAesSaWords / 4); q += kTile) s_dyn[q] = reinterpret_cast<const uint4 *>(A.sa)[q];
    {
        const uint32_t v = A.td0[tid];
#pragma unroll
        for (int t = 0; t < NTAB; ++t)
#pragma unroll
            for (int r = 0; r < REPL; ++r) s_td[t * 256 * REPL + tid * REPL + r] = t ? __builtin_amdgcn_alignbit(v, v, 32u - 8u * t) : v;
        const uint32_t b = (A.isb[tid >> 2] >> (8 * (tid & 3))) & 0xffu;
#pragma unroll
        for (int r = 0; r < REPL; ++r) s_isb[tid * REPL + r] = (uint8_t)b;
    }
    if (tid < kAesStatWords) s_tot[tid] = 0;
    const uint32_t *lsa = reinterpret_cast<const uint32_t *>(s_dyn);
    auto sa_spi = [&](uint32_t idx) -> uint32_t {               // two branches, not a pointer select (flat loads)
        if (A.sa_lds) return lsa[idx * kAesSaWords];
        return A.sa[(size_t)idx * kAesSaWords];
    };
    uint32_t cnt[5] = {0, 0, 0, 0, 0};                         // wave-uniform: packets per status
    unsigned long long blocks = 0;                             // workgroup-uniform
    // aligned dword holding arena byte o (the arena is 16-B aligned, as k_rx's windows assume)
    auto adw = [&](size_t o) -> const uint32_t * { return reinterpret_cast<const uint32_t *>(A.arena + (o & ~(size_t)3)); };
    for (uint32_t tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
        __syncthreads();                                       // the tables are staged; the last tile's arrays are read
        // ---- 1. setup ---------------------------------------------------
        const uint32_t i = tile * A.tpk + tid;
        const bool live = tid < A.tpk && i < A.n;
        const uint32_t ic = live ? i : A.n - 1;                // a lane past the tile gets a readable address
        const uint2 d = A.desc[ic];
        const uint32_t v = A.verdict[ic];
        const uint32_t an1 = A.anno[4 * (size_t)ic + 1], an2 = A.anno[4 * (size_t)ic + 2], an3 = A.anno[4 * (size_t)ic + 3];
        const uint32_t end = an1 & 0xffffu, nh = an2 & 0xffffu, ipver = (an3 >> 8) & 0xffu;
        uint32_t status = FCGPU_ESP_NOT_ESP, e0 = 0, said = 0, nblk = 0;
        if (live && (v & 0xffu) == FCGPU_R_OK && ipver == 4) {
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
                        if (sa_spi(lo + half) <= spi) lo += half;
                        len -= half;
                    }
                    uint32_t plen = (uint32_t)elen - 28u;
                    if (sa_spi(lo) != spi) {
                        status = FCGPU_ESP_NO_SA;
                    } else if (plen & 7u) {
                        status = FCGPU_ESP_UNALIGNED;
                    } else {
                        status = FCGPU_ESP_OK;
                        said = lo;
                        plen += plen & 8u;                     // 8 mod 16: the first 8 digest bytes are ciphertext too
                        nblk = plen >> 4;
                    }
                }
            }
        }
        if (live) A.status[i] = (uint8_t)status;
        s_off[tid] = d.x;
        s_sae[tid] = (e0 + 16u) | said << 16;
        // ---- 2. prefix sum of nblk ------------------------------------------
        uint32_t inc = nblk;
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) {
            const uint32_t x = __shfl_up(inc, o);
            if (lane >= (uint32_t)o) inc += x;
        }
        if (lane == kWave - 1) s_wsum[wave] = inc;
        __syncthreads();
        uint32_t wbase = 0;
#pragma unroll
        for (uint32_t w = 0; w < kTile / kWave; ++w) wbase += w < wave ? s_wsum[w] : 0u;
        s_pre[tid + 1] = wbase + inc;
        if (tid == 0) s_pre[0] = 0;
        __syncthreads();
        const uint32_t total = s_pre[kTile];
        blocks += total;
        // ---- 3..7. the passes over the flattened block list -----------------
        auto load = [&](uint32_t g) -> AesIn {
            AesIn I;
            I.act = g < total;
            I.at = 0;
            I.said = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) I.c[k] = 0;
            I.x[0] = I.x[1] = 0;
            if (I.act) {
                uint32_t j = 0;                                // the last j with pre[j] <= g: its nblk is not 0
#pragma unroll
                for (uint32_t h = kTile / 2; h; h >>= 1)
                    if (s_pre[j + h] <= g) j += h;
                const uint32_t bi = g - s_pre[j], sae = s_sae[j];
                I.said = sae >> 16;
                I.at = (size_t)s_off[j] + (sae & 0xffffu) + 16u * (size_t)bi;
                const uint32_t m = (uint32_t)I.at & 3u;
                const uint32_t *pc = adw(I.at), *px = adw(I.at - (bi ? 16 : 8));
                uint32_t q[5], y[3];
#pragma unroll
                for (int k = 0; k < 5; ++k) q[k] = pc[k];      // q[4]: at most 3 B past the block when m != 0
#pragma unroll
                for (int k = 0; k < 3; ++k) y[k] = px[k];
#pragma unroll
                for (int k = 0; k < 4; ++k) I.c[k] = __builtin_amdgcn_alignbyte(q[k + 1], q[k], m);
                I.x[0] = __builtin_amdgcn_alignbyte(y[1], y[0], m);
                I.x[1] = __builtin_amdgcn_alignbyte(y[2], y[1], m);
            }
            return I;
        };
        const uint32_t npass = (total + kTile - 1) / kTile;    // workgroup-uniform
        AesIn cur = load(tid);
        for (uint32_t p = 0; p < npass; ++p) {
            const AesIn nxt = load((p + 1) * kTile + tid);     // past the list: inactive
            uint32_t o[4] = {0, 0, 0, 0};
            if (cur.act) {
                if (A.sa_lds) aes_block<NTAB, REPL, true>(cur, s_td, s_isb, lsa, A.sa, rep, o);
                else aes_block<NTAB, REPL, false>(cur, s_td, s_isb, lsa, A.sa, rep, o);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this lane's inputs of pass p + 1 are in registers
            __syncthreads();                                   // ... and every lane's: pass p may be overwritten
            if (cur.act) aes_store(A.arena, cur.at, o);
            cur = nxt;
        }
        // ---- 8. statistics -------------------------------------------------
        cnt[0] += (uint32_t)__popcll(__ballot(live && status == FCGPU_ESP_OK));
        cnt[1] += (uint32_t)__popcll(__ballot(live && status == FCGPU_ESP_NO_SA));
        cnt[2] += (uint32_t)__popcll(__ballot(live && status == FCGPU_ESP_SHORT));
        cnt[3] += (uint32_t)__popcll(__ballot(live && status == FCGPU_ESP_UNALIGNED));
        cnt[4] += (uint32_t)__popcll(__ballot(live && status == FCGPU_ESP_NOT_ESP));
    }
    __syncthreads();
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (cnt[k]) atomicAdd(&s_tot[k], cnt[k]);
    __syncthreads();
    if (tid < 5 && s_tot[tid]) atomicAdd(A.stat + tid, (unsigned long long)s_tot[tid]);
    if (tid == 5 && blocks) atomicAdd(A.stat + 5, blocks);
}

}  // namespace fcgpu
