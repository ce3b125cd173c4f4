// aes_key.hh -- the security-association table of the ESP decryption and
// encryption stage (fcgpu_espaes_set_sas) and the AES-128 tables, built on the
// host.
//
// Semantics: IPsecAES(0) (elements/ipsec/aes.cc:69-138, decrypt branch)
// decrypts 16-byte blocks with standard AES-128 (FIPS 197). The kernel runs
// the equivalent inverse cipher of FIPS 197 section 5.3.5: per SA the 44
// words of its key schedule dw[], computed here once, and for everybody one
// 256-word table Td0 and the inverse S-box.
//
// Everything is derived from the definitions: GF(2^8) modulo x^8 + x^4 + x^3 +
// x + 1 (section 4.2) through powers of the generator 03, the S-box as the
// affine map of the multiplicative inverse (5.1.1), the key expansion (5.2),
// InvMixColumns (5.3.3). No table is typed in.
//
// Byte order: a state column is held as the little-endian load of its four
// bytes, row r in bits 8r .. 8r + 7, so the kernel needs no byte swap:
//   Td0[x] = 0e.s | 09.s << 8 | 0d.s << 16 | 0b.s << 24, s = InvSbox[x],
// is row 0's contribution to InvMixColumns(InvSubBytes(.)); rows 1..3 take
// Td0 rotated left by 8, 16, 24 bits. Round r = 1..9 of column c is
//   t[c] = Td0[s[c] & ff] ^ rol8(Td0[s[c-1] >> 8 & ff]) ^ rol16(Td0[s[c-2] >> 16 & ff])
//          ^ rol24(Td0[s[c-3] >> 24]) ^ rk[4r + c]        (columns mod 4)
// which is InvShiftRows folded into the choice of source columns.
//
// Device image: an array sorted by SPI of 192-byte records
// {spi, rk[44], pad[3]}: rk[0..3] = w[40..43], rk[4r..4r+3] =
// InvMixColumns(w[40-4r..43-4r]) for r = 1..9, rk[40..43] = w[0..3]. SPI 0 and
// duplicate SPIs are refused, as are more than kMaxSas.
//
// Encryption, IPsecAES(1) (aes.cc:115-133): the cipher of FIPS
// 197 5.1 in the same byte order, with one forward table
//   Te0[x] = 02.s | s << 8 | s << 16 | 03.s << 24, s = Sbox[x],
// row 0's contribution to MixColumns(SubBytes(.)); rows 1..3 take Te0 rotated
// left by 8, 16, 24 bits. Round r = 1..9 of column c is
//   t[c] = Te0[s[c] & ff] ^ rol8(Te0[s[c+1] >> 8 & ff]) ^ rol16(Te0[s[c+2] >> 16 & ff])
//          ^ rol24(Te0[s[c+3] >> 24]) ^ rk[4r + c]        (columns mod 4)
// (ShiftRows in the choice of source columns); the last round takes the S-box
// byte from byte 1 of the same word. The encryption records have the shape of
// the decryption ones, rk[4r + c] = w[4r + c], in the same SPI order.
// No HIP here: the library and CPU programs share this file.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "../../../include/fastclick_gpu.h"

namespace fcaes {

constexpr uint32_t kMaxSas = 65536;
constexpr uint32_t kRkWords = 44;

struct SaDev {                    // one record of the device image
    uint32_t spi;
    uint32_t rk[kRkWords];        // the equivalent inverse cipher's round keys, first round first
    uint32_t pad[3];
};
static_assert(sizeof(SaDev) == 192, "the kernel reads 48 words per SA");

struct Tables {
    uint8_t sbox[256], isbox[256];
    uint32_t td0[256];
    uint32_t te0[256];
};

constexpr uint8_t xtime(uint8_t a) { return (uint8_t)((a << 1) ^ ((a & 0x80) ? 0x1b : 0)); }
constexpr uint8_t gmul(uint8_t a, uint8_t b) {
    uint8_t p = 0;
    for (int k = 0; k < 8; ++k) {
        if (b & 1) p ^= a;
        a = xtime(a);
        b >>= 1;
    }
    return p;
}
constexpr uint8_t rotl8(uint8_t v, int r) { return (uint8_t)((v << r) | (v >> (8 - r))); }

constexpr Tables make_tables() {
    Tables t{};
    uint8_t exp[256] = {}, log[256] = {};
    uint8_t x = 1;
    for (int k = 0; k < 255; ++k) {       // 03 generates the multiplicative group
        exp[k] = x;
        log[x] = (uint8_t)k;
        x = (uint8_t)(x ^ xtime(x));
    }
    for (int v = 0; v < 256; ++v) {
        const uint8_t inv = v ? exp[(255 - log[v]) % 255] : 0;
        const uint8_t s = (uint8_t)(inv ^ rotl8(inv, 1) ^ rotl8(inv, 2) ^ rotl8(inv, 3) ^ rotl8(inv, 4) ^ 0x63);
        t.sbox[v] = s;
        t.isbox[s] = (uint8_t)v;
    }
    for (int v = 0; v < 256; ++v) {
        const uint8_t s = t.isbox[v];
        t.td0[v] = (uint32_t)gmul(s, 0x0e) | (uint32_t)gmul(s, 0x09) << 8 | (uint32_t)gmul(s, 0x0d) << 16 |
                   (uint32_t)gmul(s, 0x0b) << 24;
        const uint8_t f = t.sbox[v];
        t.te0[v] = (uint32_t)gmul(f, 0x02) | (uint32_t)f << 8 | (uint32_t)f << 16 | (uint32_t)gmul(f, 0x03) << 24;
    }
    return t;
}
constexpr Tables kTables = make_tables();

inline uint32_t rol(uint32_t x, int r) { return r ? (x << r) | (x >> (32 - r)) : x; }

// FIPS 197 5.2: the 44 words of the encryption schedule as 176 bytes, w[i] at
// bytes 4i .. 4i + 3.
inline void expand_key(const uint8_t key[16], uint8_t w[176]) {
    memcpy(w, key, 16);
    uint8_t rcon = 1;
    for (int i = 4; i < 44; ++i) {
        uint8_t t[4];
        memcpy(t, w + 4 * (i - 1), 4);
        if (i % 4 == 0) {
            const uint8_t t0 = t[0];
            t[0] = (uint8_t)(kTables.sbox[t[1]] ^ rcon);
            t[1] = kTables.sbox[t[2]];
            t[2] = kTables.sbox[t[3]];
            t[3] = kTables.sbox[t0];
            rcon = xtime(rcon);
        }
        for (int b = 0; b < 4; ++b) w[4 * i + b] = (uint8_t)(w[4 * (i - 4) + b] ^ t[b]);
    }
}

inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// InvMixColumns of one column: Td0 of the S-box undoes the table's InvSubBytes.
inline uint32_t inv_mix(uint32_t c) {
    uint32_t o = 0;
    for (int r = 0; r < 4; ++r) o ^= rol(kTables.td0[kTables.sbox[(c >> (8 * r)) & 0xff]], 8 * r);
    return o;
}

inline void dec_round_keys(const uint8_t key[16], uint32_t rk[kRkWords]) {
    uint8_t w[176];
    expand_key(key, w);
    for (int r = 0; r <= 10; ++r)
        for (int c = 0; c < 4; ++c) {
            const uint32_t v = le32(w + 16 * (10 - r) + 4 * c);
            rk[4 * r + c] = (r == 0 || r == 10) ? v : inv_mix(v);
        }
}

// One block through the image's round keys and the tables: what a lane of the
// kernel computes.
inline void decrypt_block(const uint32_t rk[kRkWords], const uint8_t in[16], uint8_t out[16]) {
    uint32_t s[4], t[4];
    for (int c = 0; c < 4; ++c) s[c] = le32(in + 4 * c) ^ rk[c];
    for (int r = 1; r < 10; ++r) {
        for (int c = 0; c < 4; ++c)
            t[c] = kTables.td0[s[c] & 0xff] ^ rol(kTables.td0[(s[(c + 3) & 3] >> 8) & 0xff], 8) ^
                   rol(kTables.td0[(s[(c + 2) & 3] >> 16) & 0xff], 16) ^ rol(kTables.td0[s[(c + 1) & 3] >> 24], 24) ^
                   rk[4 * r + c];
        memcpy(s, t, sizeof s);
    }
    for (int c = 0; c < 4; ++c) {
        const uint32_t v = ((uint32_t)kTables.isbox[s[c] & 0xff] | (uint32_t)kTables.isbox[(s[(c + 3) & 3] >> 8) & 0xff] << 8 |
                            (uint32_t)kTables.isbox[(s[(c + 2) & 3] >> 16) & 0xff] << 16 |
                            (uint32_t)kTables.isbox[s[(c + 1) & 3] >> 24] << 24) ^ rk[40 + c];
        for (int b = 0; b < 4; ++b) out[4 * c + b] = (uint8_t)(v >> (8 * b));
    }
}

// The encryption schedule: the 44 words w[] as little-endian columns.
inline void enc_round_keys(const uint8_t key[16], uint32_t rk[kRkWords]) {
    uint8_t w[176];
    expand_key(key, w);
    for (uint32_t k = 0; k < kRkWords; ++k) rk[k] = le32(w + 4 * k);
}

// One block through the encryption round keys and Te0: what a lane quad of
// k_espenc computes, column c in lane c.
inline void encrypt_block(const uint32_t rk[kRkWords], const uint8_t in[16], uint8_t out[16]) {
    uint32_t s[4], t[4];
    for (int c = 0; c < 4; ++c) s[c] = le32(in + 4 * c) ^ rk[c];
    for (int r = 1; r < 10; ++r) {
        for (int c = 0; c < 4; ++c)
            t[c] = kTables.te0[s[c] & 0xff] ^ rol(kTables.te0[(s[(c + 1) & 3] >> 8) & 0xff], 8) ^
                   rol(kTables.te0[(s[(c + 2) & 3] >> 16) & 0xff], 16) ^ rol(kTables.te0[s[(c + 3) & 3] >> 24], 24) ^
                   rk[4 * r + c];
        memcpy(s, t, sizeof s);
    }
    for (int c = 0; c < 4; ++c) {           // the S-box: bytes 1 and 2 of a Te0 word
        const uint32_t v = (((kTables.te0[s[c] & 0xff] >> 8) & 0xffu) | (kTables.te0[(s[(c + 1) & 3] >> 8) & 0xff] & 0xff00u) |
                            (kTables.te0[(s[(c + 2) & 3] >> 16) & 0xff] & 0xff0000u) |
                            ((kTables.te0[s[(c + 3) & 3] >> 24] << 8) & 0xff000000u)) ^ rk[40 + c];
        for (int b = 0; b < 4; ++b) out[4 * c + b] = (uint8_t)(v >> (8 * b));
    }
}

// The device images of n SAs, sorted by SPI: `im` for decryption and, where
// `enc` is given, the encryption records in the same order. Returns FCGPU_OK
// or FCGPU_EINVAL with `err` set; the images are written only on success.
inline int build(const fcgpu_espaes_sa *sa, uint32_t n, std::vector<SaDev> &im, std::string &err,
                 std::vector<SaDev> *enc = nullptr) {
    if (n > kMaxSas) { err = "more than 65536 SAs"; return FCGPU_EINVAL; }
    std::vector<uint32_t> order(n);
    for (uint32_t k = 0; k < n; ++k) {
        if (sa[k].spi == 0) { err = "SA " + std::to_string(k) + ": SPI 0"; return FCGPU_EINVAL; }
        order[k] = k;
    }
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return sa[x].spi < sa[y].spi; });
    for (uint32_t k = 1; k < n; ++k)
        if (sa[order[k]].spi == sa[order[k - 1]].spi) {
            err = "duplicate SPI " + std::to_string(sa[order[k]].spi);
            return FCGPU_EINVAL;
        }
    std::vector<SaDev> t(n), e(enc ? n : 0);
    for (uint32_t k = 0; k < n; ++k) {
        const fcgpu_espaes_sa &src = sa[order[k]];
        t[k].spi = src.spi;
        memset(t[k].pad, 0, sizeof t[k].pad);
        dec_round_keys(src.enc_key, t[k].rk);
        if (enc) {
            e[k] = t[k];
            enc_round_keys(src.enc_key, e[k].rk);
        }
    }
    im.swap(t);
    if (enc) enc->swap(e);
    return FCGPU_OK;
}

}  // namespace fcaes
