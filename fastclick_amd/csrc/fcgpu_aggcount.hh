// fcgpu_aggcount.hh -- k_aggcount and k_aggdump: AggregateCounter on the
// device (elements/analysis/aggcounter.{hh,cc}, AggregateCounterBase<T>::update,
// aggcounter.cc:282-322, the per-packet path of push_batch). DESIGN.md 3.9.
//
// k_aggcount is a post-pass behind k_rx on the same stream. It reads the
// batch's verdicts, hashes and (byte modes) annotations; a packet is seen iff
// its reason is FCGPU_R_OK, its key is hash & mask, its amount 1, anno.length
// or anno.length - anno.nh. Counts and totals are 64 bits. A frozen counter
// (FROZEN, set between batches) only looks keys up. Out of scope: the keywords
// AGGREGATE_FREEZE, AGGREGATE_STOP, AGGREGATE_CALL and COUNT_* (they depend on
// the packet order inside a batch), EXTRA_PACKETS / EXTRA_LENGTH annotations
// (0 here), the second always-frozen input, write_ip_file, counts_pdf, banners.
//
// Global table: next_pow2(2 * capacity) slots of {tag, count}, two 64-bit
// words in one 16-byte line. tag = key | state << 32; state 0 is empty (the
// whole word 0), so every 32-bit key, 0 and 0xffffffff included, is ordinary.
// Linear probing from a multiplicative hash. A new key claims the first empty
// slot of its chain with one 64-bit compare-and-swap to the state `pending`,
// takes a ticket from nagg and publishes `live` (ticket < capacity) or
// `refused`: a refused marker stays, so every later packet of the key is
// refused too, never a part of them. A probe that meets its own key pending
// reads the slot again: the winner takes its ticket and publishes inside the
// iteration that claimed, before the loop's only exit at its latch, so it
// never waits for a spinning lane of its own wave (in the library build it is
// not even in the same workgroup, whose keys are distinct; in the naive bench
// build equal keys do share a wave). A key that reaches an empty slot when
// nagg is already at capacity is refused without a marker, but only if the
// slot is still empty when read again after nagg: a claim comes before its
// ticket, so every claim whose ticket is below capacity is visible by then,
// nagg only grows and slots never empty, and the answer cannot change later.
// That keeps markers to the claims that race at the boundary and the chains
// short. A probe that
// wraps the whole table refuses the key. Capacity is this library's limit (the
// reference grows until memory runs out).
//
// Pre-aggregation: a workgroup takes 256-packet tiles, one packet per lane.
// Within a wave, runs of equal keys in adjacent lanes are summed by a
// segmented suffix sum over one packed word (six DPP-free shuffles) and only
// the run's first lane goes on, so a tile of one flow costs four LDS inserts,
// not 256 atomics on one bank. Run heads fold (key, amount, packets) into an
// LDS table of kAgcLds slots (64-bit tag claimed by LDS compare-and-swap,
// amount and packets by LDS adds); then each thread takes two LDS slots and
// does one global probe and one 64-bit atomic add per distinct key of the
// tile. Totals (count, seen, uncounted, nnz) stay in registers over the
// workgroup's tiles and are reduced once per workgroup.
// LDS: 512 x (8 + 4 + 4) + 4 x 4 x 8 B = 8320 B per workgroup.
#pragma once
#include "fcgpu_device.hh"

namespace fcgpu {

constexpr uint32_t kAgcLds = 512;                       // LDS slots per workgroup (2 per lane)
constexpr uint32_t kAgcMaxCapacity = 1u << 24;
constexpr unsigned long long kAgcLive = 1ull << 32, kAgcRefused = 2ull << 32, kAgcPending = 3ull << 32;
// state words (unsigned long long)
constexpr uint32_t kAgcCount = 0, kAgcSeen = 1, kAgcUncounted = 2, kAgcNagg = 3, kAgcNnz = 4, kAgcDumped = 5;
constexpr uint32_t kAgcStateWords = 8;

struct AgcArgs {
    const uint16_t *verdict;      // [n] k_rx's verdicts
    const uint32_t *hash;         // [n] ... AGGREGATE annotations
    const uint32_t *anno;         // [n] fcgpu_anno as 4 words each (byte modes; else unused)
    uint32_t n, ntiles;
    uint32_t mask;
    uint32_t mode;                // 0 packets, 1 bytes, 2 ip_bytes
    unsigned long long *tab;      // [2 * slots] {tag, count}
    unsigned long long *state;    // [kAgcStateWords]
    uint32_t shift;               // 32 - log2(slots)
    uint32_t slot_mask;           // slots - 1
    uint32_t capacity;
};

__host__ __device__ inline uint32_t agc_hash(uint32_t key) { return key * 0x9E3779B1u; }

__device__ __forceinline__ unsigned long long agc_load(const unsigned long long *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ unsigned long long wave_sum64(unsigned long long v) {
    for (int o = 32; o; o >>= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, o), hi = __shfl_xor((uint32_t)(v >> 32), o);
        v += ((unsigned long long)hi << 32) | lo;
    }
    return v;
}

// One key of a tile into the global table: true iff it has (or got) a node,
// slot = its place.
template <bool FROZEN>
__device__ __forceinline__ bool agc_probe(const AgcArgs &a, uint32_t key, uint32_t &slot) {
    uint32_t h = agc_hash(key) >> a.shift, steps = 0;
    int res = -1;                                          // undecided; the loop has one exit, at its latch
    while (res < 0) {
        unsigned long long *tag = a.tab + 2 * (size_t)h;
        const unsigned long long t = agc_load(tag);
        slot = h;
        if (t == (key | kAgcLive)) {
            res = 1;
        } else if (t == (key | kAgcRefused)) {
            res = 0;
        } else if (t == (key | kAgcPending)) {
            // its winner publishes within its own iteration: read the slot again
        } else if (t == 0) {
            if (FROZEN) {
                res = 0;
            } else if (agc_load(a.state + kAgcNagg) >= a.capacity) {
                // full: refuse only if the slot is still empty now that nagg
                // has been seen at capacity (a claim made before that is
                // visible here: the claim precedes its ticket); else look again
                if (agc_load(tag) == 0) res = 0;
            } else if (atomicCAS(tag, 0ull, key | kAgcPending) == 0) {
                const bool ok = atomicAdd(a.state + kAgcNagg, 1ull) < a.capacity;
                __hip_atomic_store(tag, key | (ok ? kAgcLive : kAgcRefused), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                res = ok;
            }                                              // else claimed meanwhile: read it again
        } else {
            h = (h + 1) & a.slot_mask;
            if (++steps > a.slot_mask) res = 0;
        }
    }
    return res != 0;
}

template <bool FROZEN>
__global__ __launch_bounds__(kTile) void k_aggcount(const AgcArgs a) {
    __shared__ unsigned long long s_tag[kAgcLds];
    __shared__ uint32_t s_amt[kAgcLds], s_pkt[kAgcLds];
    __shared__ unsigned long long s_tot[4][4];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (uint32_t k = tid; k < kAgcLds; k += kTile) {
        s_tag[k] = 0;
        s_amt[k] = 0;
        s_pkt[k] = 0;
    }
    __syncthreads();
    unsigned long long t_count = 0;
    uint32_t t_seen = 0, t_unc = 0, t_nnz = 0;
    for (uint32_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const uint32_t i = tile * kTile + tid;
        bool ok = false;
        uint32_t key = 0, amt = 1;
        if (i < a.n) {
            ok = (a.verdict[i] & 0xff) == FCGPU_R_OK;
            key = a.hash[i] & a.mask;
            if (a.mode) {                                   // launch-uniform
                // word 1: length | vlan_tci << 16, word 2: nh | th << 16
                const uint32_t len = a.anno[4 * (size_t)i + 1] & 0xffff, nh = a.anno[4 * (size_t)i + 2] & 0xffff;
                amt = a.mode == 2 ? (len > nh ? len - nh : 0u) : len;
            }
        }
        t_seen += ok;
#ifdef FCGPU_AGGCOUNT_NAIVE
        // bench-only build (scripts/aggcount_bench.py): one global probe and
        // one atomic per packet, no wave combine, no LDS stage
        if (ok) {
            uint32_t slot;
            if (agc_probe<FROZEN>(a, key, slot)) {
                const unsigned long long old = atomicAdd(a.tab + 2 * (size_t)slot + 1, (unsigned long long)amt);
                t_nnz += amt && old == 0;
                t_count += amt;
            } else {
                ++t_unc;
            }
        }
        continue;
#endif
        // runs of equal keys in adjacent lanes: the head gets the run's sums.
        // v = amount (< 2^22 over a wave) | packets << 24
        const uint32_t pkey = __shfl_up(key, 1);
        const uint64_t mok = __ballot(ok);
        const bool pok = lane && ((mok >> (lane - 1)) & 1);
        const bool head = !ok || !pok || pkey != key;
        const uint64_t heads = __ballot(head);
        uint32_t v = ok ? (amt | (1u << 24)) : 0u;
        const uint64_t above = lane == 63 ? 0ull : heads >> (lane + 1);   // bit j: lane + 1 + j is a head
        for (uint32_t d = 1; d < 64; d <<= 1) {
            const uint32_t o = __shfl_down(v, d);
            if (lane + d < 64 && (above & ((1ull << d) - 1)) == 0) v += o;
        }
        if (ok && head) {
            const unsigned long long mine = key | kAgcLive;
            for (uint32_t h = agc_hash(key) >> 23;; h = (h + 1) & (kAgcLds - 1)) {
                const unsigned long long old = atomicCAS(&s_tag[h], 0ull, mine);
                if (old == 0 || old == mine) {
                    atomicAdd(&s_amt[h], v & 0xffffffu);
                    atomicAdd(&s_pkt[h], v >> 24);
                    break;
                }
            }
        }
        __syncthreads();
        // one probe and one add per distinct key of the tile
        for (uint32_t k = tid; k < kAgcLds; k += kTile) {
            const unsigned long long t = s_tag[k];
            if (t == 0) continue;
            const uint32_t amount = s_amt[k], pk = s_pkt[k];
            s_tag[k] = 0;
            s_amt[k] = 0;
            s_pkt[k] = 0;
            uint32_t slot;
            if (agc_probe<FROZEN>(a, (uint32_t)t, slot)) {
                const unsigned long long old = atomicAdd(a.tab + 2 * (size_t)slot + 1, (unsigned long long)amount);
                t_nnz += amount && old == 0;
                t_count += amount;
            } else {
                t_unc += pk;
            }
        }
        __syncthreads();
    }
    // totals: per wave, then per workgroup, one add each
    const unsigned long long w[4] = {wave_sum64(t_count), wave_sum64(t_seen), wave_sum64(t_unc), wave_sum64(t_nnz)};
    if (lane == 0)
        for (int k = 0; k < 4; ++k) s_tot[wave][k] = w[k];
    __syncthreads();
    if (tid < 4) {
        const unsigned long long sum = s_tot[0][tid] + s_tot[1][tid] + s_tot[2][tid] + s_tot[3][tid];
        const uint32_t word = tid == 0 ? kAgcCount : tid == 1 ? kAgcSeen : tid == 2 ? kAgcUncounted : kAgcNnz;
        if (sum) atomicAdd(a.state + word, sum);
    }
}

// Live slots with a non-zero count -> records {agg, 0, count}, unordered: a
// wave ballot and one atomic per wave for the output offset. rec holds max
// records; state[kAgcDumped] (cleared by the caller) ends as the number found.
__global__ __launch_bounds__(kTile) void k_aggdump(const unsigned long long *tab, uint32_t slots, uint4 *rec,
                                                  uint32_t max, unsigned long long *state) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t stride = gridDim.x * kTile;
    for (uint32_t base = blockIdx.x * kTile; base < slots; base += stride) {      // slots: a multiple of kTile or < kTile
        const uint32_t s = base + threadIdx.x;
        unsigned long long tag = 0, cnt = 0;
        if (s < slots) {
            tag = tab[2 * (size_t)s];
            cnt = tab[2 * (size_t)s + 1];
        }
        const bool out = (tag >> 32) == (kAgcLive >> 32) && cnt != 0;
        const uint64_t m = __ballot(out);
        if (!m) continue;
        uint32_t off = 0;
        if (lane == 0) off = (uint32_t)atomicAdd(state + kAgcDumped, (unsigned long long)__popcll(m));
        off = __shfl(off, 0) + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (out && off < max) rec[off] = make_uint4((uint32_t)tag, 0u, (uint32_t)cnt, (uint32_t)(cnt >> 32));
    }
}

}  // namespace fcgpu
