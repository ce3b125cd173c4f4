// fcgpu_espenc.hh -- k_espenc: IPsecAES(1) on the device (elements/ipsec/
// aes.cc:69-138, encrypt branch, the chaining of lines 115-133: AES-128 with
// the first 8 bytes of a block XORed with the first 8 bytes of the previous
// ciphertext block, the IV for block 0), a post-pass behind k_rx and behind
// k_espauth on the same stream, encrypting in place in the arena. Semantics:
// include/fastclick_gpu.h; DESIGN.md 3.12.
//
// Unlike decryption (fcgpu_espaes.hh) a packet is one serial chain: block i
// needs the output of block i - 1. The parallelism is across packets and
// inside one block: four lanes per packet, lane c of the quad holding state
// column c, a wave serving 16 packets. Per tile of `tpk` packets (256, fewer
// when the batch has too few packets to fill the device) a workgroup of 256
// lanes does:
//   1. Setup, one lane per packet, k_espaes's step 1 word for word: status,
//      the SA by a binary search of uniform depth (encryption image in LDS up
//      to 16 KB, else global), nblk. The status byte goes to the packet's own
//      index.
//   2. Order (SORT): a counting sort of the tile by min(nblk, 63) in LDS,
//      longest first, as k_espauth orders by its block count: a wave runs to
//      the longest of its 16 packets. The bin bases are one suffix scan by
//      wave 0. A tile whose packets all have one nblk keeps arrival order.
//      Packets with nblk == 0 sort last and take no group. Without SORT
//      every packet of the tile takes a slot in arrival order.
//   3. Waves take groups of 16 sorted slots (wave w: groups w, w + 4, ...).
//      Per group lane c of quad q serves slot 16 g + q: it preloads its 11
//      round-key words rk[4r + c] into registers, loads the IV word (lanes 0
//      and 1) and column c of block 0.
//   4. Per block: column c of block i + 1 is loaded (two aligned dwords, one
//      v_alignbyte_b32; the quad shares the misalignment) before block i's
//      rounds. Lanes 0 and 1 XOR the chain word in: the IV word, afterwards
//      their own previous output column, kept in a register. No chain byte
//      is re-read from memory and no lane reads a byte another lane of the
//      kernel writes (the aligned dwords may touch such a byte; the funnel
//      shift discards it), so in-place writing raises no ordering question.
//   5. A round (1..9): lane c needs byte 0 of its own column and bytes 1, 2,
//      3 of columns c + 1, c + 2, c + 3: three DPP quad_perm moves (the quad
//      rotated by 1, 2, 3), four Te0 lookups in LDS, three v_alignbit_b32
//      rotates, the XORs with the register-resident round key. The last round
//      takes the S-box byte from bytes 1 / 2 of the same Te0 words. No LDS
//      round trip and no ds_bpermute for the exchange. All 64 lanes run the
//      rounds of every step up to the wave's longest packet (the DPP moves
//      sit in uniform control flow); loads and stores are predicated.
//   6. Each lane stores its own four bytes by the address's low two bits: one
//      dword, two shorts, or byte + short + byte. Nothing else is written.
//   7. Statistics by ballot, one atomic per non-zero counter per workgroup.
// LDS per workgroup: Te0 1 KB, 3 KB of slot arrays, 0.3 KB of bins and
// totals, and the SA image (<= 16 KB, dynamic).
#pragma once
#include "fcgpu_espaes.hh"

namespace fcgpu {

constexpr uint32_t kEncBins = 64;               // min(nblk, 63): a 1008-byte payload and longer share the top bin
constexpr uint32_t kEncGroup = 16;              // packets a wave serves at once
constexpr uint32_t kEncWgPerCu = 7;             // workgroups per CU the launch asks for: the kernel's 7 waves a SIMD
constexpr uint32_t kEncMinTile = 64;            // one group per wave

struct EncArgs {
    uint8_t *arena;
    const uint2 *desc;
    const uint16_t *verdict;      // [n] k_rx's verdicts
    const uint32_t *anno;         // [n] fcgpu_anno as 4 words each
    uint32_t n, ntiles;
    uint32_t tpk;                 // packets per tile: a power of two, kEncGroup <= tpk <= kTile
    const uint32_t *sa;           // [nsa * kAesSaWords] encryption records, sorted by spi
    uint32_t nsa;                 // >= 1
    uint32_t sa_lds;              // the image is staged in (dynamic) LDS
    const uint32_t *te0;          // [256] Te0
    uint8_t *status;              // [n]
    unsigned long long *stat;     // [kAesStatWords]
};

// The quad rotated by R: lane c gets lane (c + R) & 3's value.
template <int R> __device__ __forceinline__ uint32_t enc_quad_rot(uint32_t v) {
    constexpr int ctrl = ((R) & 3) | ((R + 1) & 3) << 2 | ((R + 2) & 3) << 4 | ((R + 3) & 3) << 6;   // quad_perm
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, 0xf, 0xf, true);
}

// One block: the lane's column `s` (chain word already XORed in) through the
// ten rounds with the lane's round-key words; every lane of the quad calls it.
__device__ __forceinline__ uint32_t enc_block(uint32_t s, const uint32_t (&rk)[11], const uint32_t *s_te) {
    s ^= rk[0];
#pragma unroll
    for (int r = 1; r < 10; ++r) {
        const uint32_t s1 = enc_quad_rot<1>(s), s2 = enc_quad_rot<2>(s), s3 = enc_quad_rot<3>(s);
        const uint32_t t0 = s_te[s & 0xffu], t1 = s_te[(s1 >> 8) & 0xffu], t2 = s_te[(s2 >> 16) & 0xffu], t3 = s_te[s3 >> 24];
        s = t0 ^ __builtin_amdgcn_alignbit(t1, t1, 24u) ^ __builtin_amdgcn_alignbit(t2, t2, 16u) ^
            __builtin_amdgcn_alignbit(t3, t3, 8u) ^ rk[r];
    }
    const uint32_t s1 = enc_quad_rot<1>(s), s2 = enc_quad_rot<2>(s), s3 = enc_quad_rot<3>(s);
    const uint32_t t0 = s_te[s & 0xffu], t1 = s_te[(s1 >> 8) & 0xffu], t2 = s_te[(s2 >> 16) & 0xffu], t3 = s_te[s3 >> 24];
    // Te0's bytes 1 and 2 are the S-box byte
    return (((t0 >> 8) & 0xffu) | (t1 & 0xff00u) | (t2 & 0xff0000u) | ((t3 << 8) & 0xff000000u)) ^ rk[10];
}

// The lane's four bytes to arena + at by naturally aligned stores. The empty
// asm statements are compiler barriers only: without them the pieces are merged
// into one unaligned dword store.
__device__ __forceinline__ void enc_store(uint8_t *arena, size_t at, uint32_t o) {
    uint8_t *p = arena + at;
    const uint32_t m = (uint32_t)at & 3u;
    if (m == 0) {
        *reinterpret_cast<uint32_t *>(p) = o;
    } else if (m == 2) {
        *reinterpret_cast<uint16_t *>(p) = (uint16_t)o;
        asm volatile("" ::: "memory");
        *reinterpret_cast<uint16_t *>(p + 2) = (uint16_t)(o >> 16);
    } else {
        p[0] = (uint8_t)o;
        asm volatile("" ::: "memory");
        *reinterpret_cast<uint16_t *>(p + 1) = (uint16_t)(o >> 8);
        asm volatile("" ::: "memory");
        p[3] = (uint8_t)(o >> 24);
    }
}

template <bool SORT>
__global__ __launch_bounds__(kTile) void k_espenc(const EncArgs A) {
    extern __shared__ uint4 s_dyn[];                           // the SA image (A.sa_lds)
    __shared__ uint32_t s_te[256];
    __shared__ uint32_t s_off[kTile];                          // by sorted slot: frame offset
    __shared__ uint32_t s_sae[kTile];                          // e0 + 16 | SA index << 16
    __shared__ uint32_t s_nb[kTile];                           // nblk
    __shared__ uint32_t s_bin[kEncBins + 1];                   // counts, then the bins' bases; word kEncBins: the first packet's nblk
    __shared__ uint32_t s_tot[kAesStatWords];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t col = lane & 3u, quad = lane >> 2;
    if (A.sa_lds)
        for (uint32_t q = tid; q < A.nsa * (kAesSaWords / 4); q += kTile) s_dyn[q] = reinterpret_cast<const uint4 *>(A.sa)[q];
    s_te[tid] = A.te0[tid];
    if (tid < kAesStatWords) s_tot[tid] = 0;
    const uint32_t *lsa = reinterpret_cast<const uint32_t *>(s_dyn);
    auto sa_word = [&](uint32_t idx, uint32_t k) -> uint32_t {  // two branches, not a pointer select (flat loads)
        if (A.sa_lds) return lsa[idx * kAesSaWords + k];
        return A.sa[(size_t)idx * kAesSaWords + k];
    };
    uint32_t cnt[5] = {0, 0, 0, 0, 0};                         // wave-uniform: packets per status
    unsigned long long blocks = 0;                             // wave-uniform: this wave's packets' blocks
    // aligned dword holding arena byte o (the arena is 16-B aligned, as k_rx's windows assume)
    auto adw = [&](size_t o) -> const uint32_t * { return reinterpret_cast<const uint32_t *>(A.arena + (o & ~(size_t)3)); };
    for (uint32_t tile = blockIdx.x; tile < A.ntiles; tile += gridDim.x) {
        __syncthreads();                                       // the tables are staged; the last tile's slots are read
        // ---- 1. setup (k_espaes step 1) -----------------------------------
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
                        if (sa_word(lo + half, 0) <= spi) lo += half;
                        len -= half;
                    }
                    uint32_t plen = (uint32_t)elen - 28u;
                    if (sa_word(lo, 0) != spi) {
                        status = FCGPU_ESP_NO_SA;
                    } else if (plen & 7u) {
                        status = FCGPU_ESP_UNALIGNED;
                    } else {
                        status = FCGPU_ESP_OK;
                        said = lo;
                        plen += plen & 8u;                     // 8 mod 16: the first 8 digest bytes are encrypted too
                        nblk = plen >> 4;
                    }
                }
            }
        }
        if (live) A.status[i] = (uint8_t)status;
        // ---- 2. order by nblk, longest first --------------------------------
        uint32_t pos = tid, nact = A.tpk;                      // nact: slots that take a group (workgroup-uniform)
        if (SORT) {
            const uint32_t bin = nblk < kEncBins - 1 ? nblk : kEncBins - 1;
            if (tid < kEncBins) s_bin[tid] = 0u;
            if (tid == 0) s_bin[kEncBins] = nblk;              // the tile's first packet: always live
            __syncthreads();
            const uint32_t first = s_bin[kEncBins];
            if (__syncthreads_and(!live || nblk == first)) {   // one nblk throughout: arrival order
                nact = first ? A.tpk : 0u;
            } else {
                const uint32_t rank = atomicAdd(&s_bin[bin], 1u);
                __syncthreads();
                const uint32_t zero = s_bin[0];
                __syncthreads();
                if (wave == 0) {                               // base of bin b: the packets in the bins above it
                    const uint32_t own = s_bin[lane];
                    uint32_t suf = own;
#pragma unroll
                    for (int o = 1; o < kWave; o <<= 1) {
                        const uint32_t x = __shfl_down(suf, o);
                        if (lane + (uint32_t)o < kWave) suf += x;
                    }
                    s_bin[lane] = suf - own;
                }
                __syncthreads();
                pos = s_bin[bin] + rank;
                nact = kTile - zero;                           // lanes past the tile have nblk 0
            }
        }
        s_off[pos] = d.x;
        s_sae[pos] = (e0 + 16u) | said << 16;
        s_nb[pos] = nblk;
        __syncthreads();
        // ---- 3..6. groups of 16 slots, a quad per packet --------------------
        for (uint32_t g = wave; g * kEncGroup < nact; g += kTile / kWave) {
            const uint32_t slot = g * kEncGroup + quad;
            const bool has = slot < nact;
            const uint32_t nb = has ? s_nb[slot] : 0u, sae = s_sae[slot], sid = has ? sae >> 16 : 0u;
            // arena offset of this lane's column of block 0
            const size_t at0 = (size_t)s_off[slot] + (sae & 0xffffu) + 4u * col;
            const uint32_t m = (uint32_t)at0 & 3u;
            uint32_t maxnb = nb;
#pragma unroll
            for (int o = 4; o < kWave; o <<= 1) {
                const uint32_t x = __shfl_xor(maxnb, o);
                maxnb = x > maxnb ? x : maxnb;
            }
            maxnb = __builtin_amdgcn_readfirstlane(maxnb);
            uint32_t rk[11];
#pragma unroll
            for (int r = 0; r < 11; ++r) rk[r] = sa_word(sid, 1 + 4 * r + col);
            uint32_t chain = 0, q0 = 0, q1 = 0;                // q0, q1: the raw dwords over the next column
            if (nb) {
                if (col < 2) {                                 // the IV word: 8 bytes in front of block 0
                    const uint32_t *pi = adw(at0 - 8);
                    chain = __builtin_amdgcn_alignbyte(pi[1], pi[0], m);
                }
                const uint32_t *pc = adw(at0);                 // pc[1]: at most 3 B past the column when m != 0
                q0 = pc[0];
                q1 = pc[1];
            }
            for (uint32_t b = 0; b < maxnb; ++b) {             // wave-uniform
                const uint32_t cur = __builtin_amdgcn_alignbyte(q1, q0, m);
                if (b + 1 < nb) {                              // in flight over block b's rounds
                    const uint32_t *pc = adw(at0 + 16 * (size_t)(b + 1));
                    q0 = pc[0];
                    q1 = pc[1];
                }
                const uint32_t o = enc_block(cur ^ chain, rk, s_te);
                if (b < nb) {
                    enc_store(A.arena, at0 + 16 * (size_t)b, o);
                    chain = col < 2 ? o : 0u;
                }
            }
        }
        // ---- 7. statistics -------------------------------------------------
        cnt[0] += (uint32_t)__popcll(__ballot(live && status == FCGPU_ESP_OK));
        cnt[1] += (uint32_t)__popcll(__ballot(live && status == FCGPU_ESP_NO_SA));
        cnt[2] += (uint32_t)__popcll(__ballot(live && status == FCGPU_ESP_SHORT));
        cnt[3] += (uint32_t)__popcll(__ballot(live && status == FCGPU_ESP_UNALIGNED));
        cnt[4] += (uint32_t)__popcll(__ballot(live && status == FCGPU_ESP_NOT_ESP));
        uint32_t wb = nblk;                                    // the blocks of this wave's 64 setup packets: < 2^18
#pragma unroll
        for (int o = 1; o < kWave; o <<= 1) wb += __shfl_xor(wb, o);
        blocks += wb;
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < 5; ++k)
            if (cnt[k]) atomicAdd(&s_tot[k], cnt[k]);
        if (blocks) atomicAdd(A.stat + 5, blocks);
    }
    __syncthreads();
    if (tid < 5 && s_tot[tid]) atomicAdd(A.stat + tid, (unsigned long long)s_tot[tid]);
}

}  // namespace fcgpu
