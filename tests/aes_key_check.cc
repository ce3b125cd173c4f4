// aes_key_check.cc -- sanitizer run of host/aes_key.hh (TEST INFRASTRUCTURE, CPU only, built by
// tests/test_espaes_host.py): key expansion against FIPS 197 A.1, decryption through the image against C.1,
// seeded random tables against a byte-wise FIPS 197 5.1 cipher written here, the refusals.
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include "../fastclick_amd/csrc/host/aes_key.hh"

#define CHECK(c) \
    do { if (!(c)) { fprintf(stderr, "aes_key_check: failed at %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static std::vector<uint8_t> hex(const char *s) {
    std::vector<uint8_t> v;
    for (; s[0] && s[1]; s += 2) v.push_back((uint8_t)strtoul(std::string(s, 2).c_str(), nullptr, 16));
    return v;
}

// FIPS 197 5.1, byte by byte: state byte (row r, column c) at st[4c + r].
static void encrypt_plain(const uint8_t key[16], const uint8_t in[16], uint8_t out[16]) {
    uint8_t w[176], st[16], t[16];
    fcaes::expand_key(key, w);
    for (int k = 0; k < 16; ++k) st[k] = in[k] ^ w[k];
    for (int r = 1; r <= 10; ++r) {
        for (int c = 0; c < 4; ++c)
            for (int q = 0; q < 4; ++q) t[4 * c + q] = fcaes::kTables.sbox[st[4 * ((c + q) & 3) + q]];   // SubBytes, ShiftRows
        for (int c = 0; c < 4 && r < 10; ++c) {                                                          // MixColumns
            const uint8_t a[4] = {t[4 * c], t[4 * c + 1], t[4 * c + 2], t[4 * c + 3]};
            for (int q = 0; q < 4; ++q)
                t[4 * c + q] = fcaes::gmul(a[q], 2) ^ fcaes::gmul(a[(q + 1) & 3], 3) ^ a[(q + 2) & 3] ^ a[(q + 3) & 3];
        }
        for (int k = 0; k < 16; ++k) st[k] = t[k] ^ w[16 * r + k];
    }
    memcpy(out, st, 16);
}

int main() {
    CHECK(fcaes::kTables.sbox[0x00] == 0x63 && fcaes::kTables.sbox[0x53] == 0xed && fcaes::kTables.isbox[0xed] == 0x53);
    // Appendix A.1: w4, w5, w43 of the key 2b7e1516 28aed2a6 abf71588 09cf4f3c
    uint8_t w[176];
    fcaes::expand_key(hex("2b7e151628aed2a6abf7158809cf4f3c").data(), w);
    CHECK(!memcmp(w + 16, hex("a0fafe1788542cb1").data(), 8) && !memcmp(w + 4 * 43, hex("b6630ca6").data(), 4));
    CHECK(!memcmp(w + 4 * 20, hex("d4d1c6f87c839d87caf2b8bc11f915bc").data(), 16));
    // Appendix C.1, both ways
    const auto key = hex("000102030405060708090a0b0c0d0e0f"), pt = hex("00112233445566778899aabbccddeeff"),
               ct = hex("69c4e0d86a7b0430d8cdb78070b4c55a");
    uint8_t out[16];
    uint32_t rk[fcaes::kRkWords];
    encrypt_plain(key.data(), pt.data(), out);
    CHECK(!memcmp(out, ct.data(), 16));
    fcaes::dec_round_keys(key.data(), rk);
    fcaes::decrypt_block(rk, ct.data(), out);
    CHECK(!memcmp(out, pt.data(), 16));

    std::mt19937 rng(12345);
    std::vector<fcaes::SaDev> im;
    std::string err;
    for (uint32_t n : {0u, 1u, 2u, 85u, 86u, 3000u}) {
        std::vector<fcgpu_espaes_sa> sa(n);
        for (uint32_t k = 0; k < n; ++k) {
            sa[k].spi = 1 + k * 7919u % 100003u;      // distinct, unsorted
            for (auto &b : sa[k].enc_key) b = (uint8_t)rng();
        }
        CHECK(fcaes::build(sa.data(), n, im, err) == FCGPU_OK && im.size() == n);
        for (uint32_t k = 0; k < n; ++k) {
            CHECK(k == 0 || im[k - 1].spi < im[k].spi);
            const fcgpu_espaes_sa *src = nullptr;
            for (const auto &s : sa)
                if (s.spi == im[k].spi) src = &s;
            CHECK(src && !im[k].pad[0] && !im[k].pad[1] && !im[k].pad[2]);
            uint8_t p[16], c[16], d[16];
            for (auto &b : p) b = (uint8_t)rng();
            encrypt_plain(src->enc_key, p, c);
            fcaes::decrypt_block(im[k].rk, c, d);
            CHECK(!memcmp(p, d, 16));
        }
        // refusals leave the image as it is
        if (n >= 2) {
            const std::vector<fcaes::SaDev> keep = im;
            std::vector<fcgpu_espaes_sa> bad = sa;
            bad[n - 1].spi = bad[0].spi;
            CHECK(fcaes::build(bad.data(), n, im, err) == FCGPU_EINVAL && err.find("duplicate") != std::string::npos);
            bad = sa;
            bad[n / 2].spi = 0;
            CHECK(fcaes::build(bad.data(), n, im, err) == FCGPU_EINVAL && err.find("SPI 0") != std::string::npos);
            CHECK(im.size() == keep.size() && !memcmp(im.data(), keep.data(), keep.size() * sizeof keep[0]));
        }
    }
    std::vector<fcgpu_espaes_sa> many(fcaes::kMaxSas + 1);
    for (uint32_t k = 0; k < many.size(); ++k) many[k].spi = k + 1;
    CHECK(fcaes::build(many.data(), (uint32_t)many.size(), im, err) == FCGPU_EINVAL);
    CHECK(fcaes::build(many.data(), fcaes::kMaxSas, im, err) == FCGPU_OK && im.size() == fcaes::kMaxSas);
    printf("aes_key_check ok\n");
    return 0;
}
