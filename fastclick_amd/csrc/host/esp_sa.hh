// esp_sa.hh -- the security-association table of the ESP authentication stage
// (fcgpu_espauth_set_sas), built on the host.
//
// Semantics: IPsecAuthHMACSHA1 (elements/ipsec/hmacsha1.cc:61-96) runs HMAC
// (hmac.cc:147-159, plain HMAC-SHA1) with the SA's 16-byte authentication key
// and keeps the first 12 bytes. HMAC(K, m) = H((K ^ opad) || H((K ^ ipad) || m))
// (RFC 2104) and K ^ ipad, K ^ opad each fill exactly one 64-byte SHA-1 block,
// so the state after compressing each of them depends on the key alone: the
// two midstates, 2 x 5 words, are computed here once per SA and a packet's
// HMAC costs ceil((len + 9) / 64) + 1 compressions instead of two more.
//
// Device image: an array sorted by SPI of 48-byte records
// {spi, inner[5], outer[5], 0}; the kernel finds a packet's SA by binary
// search. SPI 0 and duplicate SPIs are refused, as are more than kMaxSas.
//
// The SHA-1 compression function is written from FIPS 180-1 section 7
// (method 1, an 80-word schedule). No HIP here: the library and CPU programs
// share this file.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../../include/fastclick_gpu.h"

namespace fcesp {

constexpr uint32_t kMaxSas = 65536;
constexpr uint32_t kInit[5] = {0x67452301u, 0xEFCDAB89u, 0x98BADCFEu, 0x10325476u, 0xC3D2E1F0u};

struct SaDev {                    // one record of the device image
    uint32_t spi;
    uint32_t inner[5], outer[5];  // SHA-1 states after key ^ ipad, key ^ opad
    uint32_t pad;
};
static_assert(sizeof(SaDev) == 48, "the kernel reads 12 words per SA");

inline uint32_t rol(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }

// One 64-byte block, given as 16 big-endian words, into the state h.
inline void sha1_compress(uint32_t h[5], const uint32_t blk[16]) {
    uint32_t w[80];
    for (int t = 0; t < 16; ++t) w[t] = blk[t];
    for (int t = 16; t < 80; ++t) w[t] = rol(w[t - 3] ^ w[t - 8] ^ w[t - 14] ^ w[t - 16], 1);
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
    for (int t = 0; t < 80; ++t) {
        uint32_t f, k;
        if (t < 20) { f = (b & c) | (~b & d); k = 0x5A827999u; }
        else if (t < 40) { f = b ^ c ^ d; k = 0x6ED9EBA1u; }
        else if (t < 60) { f = (b & c) | (b & d) | (c & d); k = 0x8F1BBCDCu; }
        else { f = b ^ c ^ d; k = 0xCA62C1D6u; }
        const uint32_t tmp = rol(a, 5) + f + e + w[t] + k;
        e = d; d = c; c = rol(b, 30); b = a; a = tmp;
    }
    h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e;
}

// SHA-1 of msg[0, n) continued from state h, which has already absorbed
// `before` bytes (a multiple of 64); the digest as 20 big-endian bytes.
inline void sha1_finish(uint32_t h[5], uint64_t before, const uint8_t *msg, size_t n, uint8_t out[20]) {
    uint8_t buf[64];
    uint32_t blk[16];
    auto block = [&](const uint8_t *p) {
        for (int j = 0; j < 16; ++j)
            blk[j] = (uint32_t)p[4 * j] << 24 | (uint32_t)p[4 * j + 1] << 16 | (uint32_t)p[4 * j + 2] << 8 | p[4 * j + 3];
        sha1_compress(h, blk);
    };
    size_t i = 0;
    for (; i + 64 <= n; i += 64) block(msg + i);
    const size_t rest = n - i;
    memset(buf, 0, sizeof buf);
    if (rest) memcpy(buf, msg + i, rest);
    buf[rest] = 0x80;
    if (rest >= 56) {             // no room for the length: one more block
        block(buf);
        memset(buf, 0, sizeof buf);
    }
    const uint64_t bits = (before + n) * 8;
    for (int j = 0; j < 8; ++j) buf[56 + j] = (uint8_t)(bits >> (8 * (7 - j)));
    block(buf);
    for (int j = 0; j < 5; ++j)
        for (int b = 0; b < 4; ++b) out[4 * j + b] = (uint8_t)(h[j] >> (8 * (3 - b)));
}

inline void sha1(const uint8_t *msg, size_t n, uint8_t out[20]) {
    uint32_t h[5];
    memcpy(h, kInit, sizeof h);
    sha1_finish(h, 0, msg, n, out);
}

// The two HMAC midstates of a key of at most 64 bytes (a longer key is hashed
// first, RFC 2104; the SA keys here are 16 bytes). false: klen > 64.
inline bool hmac_midstates(const uint8_t *key, size_t klen, uint32_t inner[5], uint32_t outer[5]) {
    if (klen > 64) return false;
    uint32_t blk[16];
    for (int pass = 0; pass < 2; ++pass) {
        uint8_t pad[64];
        memset(pad, pass ? 0x5c : 0x36, sizeof pad);
        for (size_t j = 0; j < klen; ++j) pad[j] ^= key[j];
        for (int j = 0; j < 16; ++j)
            blk[j] = (uint32_t)pad[4 * j] << 24 | (uint32_t)pad[4 * j + 1] << 16 | (uint32_t)pad[4 * j + 2] << 8 | pad[4 * j + 3];
        uint32_t *h = pass ? outer : inner;
        memcpy(h, kInit, 5 * sizeof(uint32_t));
        sha1_compress(h, blk);
    }
    return true;
}

// HMAC-SHA1 from the midstates: what the kernel computes per packet.
inline void hmac_from_midstates(const uint32_t inner[5], const uint32_t outer[5], const uint8_t *msg, size_t n,
                                uint8_t out[20]) {
    uint32_t h[5];
    uint8_t d[20];
    memcpy(h, inner, sizeof h);
    sha1_finish(h, 64, msg, n, d);
    memcpy(h, outer, sizeof h);
    sha1_finish(h, 64, d, 20, out);
}

// The device image of n SAs, sorted by SPI. Returns FCGPU_OK or FCGPU_EINVAL
// with `err` set; `im` is written only on success.
inline int build(const fcgpu_esp_sa *sa, uint32_t n, std::vector<SaDev> &im, std::string &err) {
    if (n > kMaxSas) { err = "more than 65536 SAs"; return FCGPU_EINVAL; }
    std::vector<SaDev> t(n);
    for (uint32_t k = 0; k < n; ++k) {
        if (sa[k].spi == 0) { err = "SA " + std::to_string(k) + ": SPI 0"; return FCGPU_EINVAL; }
        t[k].spi = sa[k].spi;
        t[k].pad = 0;
        hmac_midstates(sa[k].auth_key, sizeof sa[k].auth_key, t[k].inner, t[k].outer);
    }
    std::sort(t.begin(), t.end(), [](const SaDev &x, const SaDev &y) { return x.spi < y.spi; });
    for (uint32_t k = 1; k < n; ++k)
        if (t[k].spi == t[k - 1].spi) { err = "duplicate SPI " + std::to_string(t[k].spi); return FCGPU_EINVAL; }
    im.swap(t);
    return FCGPU_OK;
}

}  // namespace fcesp
