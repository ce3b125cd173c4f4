// aes_enc_key_check.cc -- sanitizer run of the encryption half of host/aes_key.hh (TEST INFRASTRUCTURE, CPU only,
// built by tests/test_espenc_host.py): Te0 against its definition, enc_round_keys + encrypt_block on FIPS 197 C.1 and
// A.1, encrypt then decrypt as the identity, the decryption image unchanged by the two-image build.
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include "../fastclick_amd/csrc/host/aes_key.hh"

#define CHECK(c) \
    do { if (!(c)) { fprintf(stderr, "aes_enc_key_check: failed at %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

static std::vector<uint8_t> hex(const char *s) {
    std::vector<uint8_t> v;
    for (; s[0] && s[1]; s += 2) v.push_back((uint8_t)strtoul(std::string(s, 2).c_str(), nullptr, 16));
    return v;
}

int main() {
    for (int x = 0; x < 256; ++x) {
        const uint8_t s = fcaes::kTables.sbox[x];
        const uint32_t want = (uint32_t)fcaes::gmul(s, 2) | (uint32_t)s << 8 | (uint32_t)s << 16 | (uint32_t)fcaes::gmul(s, 3) << 24;
        CHECK(fcaes::kTables.te0[x] == want && (uint8_t)(fcaes::gmul(s, 2) ^ s) == fcaes::gmul(s, 3));
    }
    CHECK(fcaes::kTables.te0[0] == 0xa56363c6u);      // Sbox[0] = 63: c6 63 63 a5
    // Appendix A.1: the schedule's words as little-endian columns
    uint32_t rk[fcaes::kRkWords], dk[fcaes::kRkWords];
    fcaes::enc_round_keys(hex("2b7e151628aed2a6abf7158809cf4f3c").data(), rk);
    CHECK(rk[0] == 0x16157e2bu && rk[4] == 0x17fefaa0u && rk[5] == 0xb12c5488u && rk[43] == 0xa60c63b6u);
    const auto key = hex("000102030405060708090a0b0c0d0e0f"), pt = hex("00112233445566778899aabbccddeeff"),
               ct = hex("69c4e0d86a7b0430d8cdb78070b4c55a");
    uint8_t out[16];
    fcaes::enc_round_keys(key.data(), rk);
    fcaes::encrypt_block(rk, pt.data(), out);
    CHECK(!memcmp(out, ct.data(), 16));
    std::mt19937 rng(4321);
    // both images from one list of seeded random keys: the decryption one is what the one-image build gives, the
    // encryption one has the same SPIs in the same order; encrypt then decrypt is the identity
    std::string err;
    for (uint32_t n : {0u, 1u, 86u, 3000u}) {
        std::vector<fcgpu_espaes_sa> sa(n);
        for (uint32_t k = 0; k < n; ++k) {
            sa[k].spi = 1 + k * 7919u % 100003u;      // distinct, unsorted
            for (auto &b : sa[k].enc_key) b = (uint8_t)rng();
        }
        std::vector<fcaes::SaDev> one, dec, enc;
        CHECK(fcaes::build(sa.data(), n, one, err) == FCGPU_OK && fcaes::build(sa.data(), n, dec, err, &enc) == FCGPU_OK);
        CHECK(one.size() == n && dec.size() == n && enc.size() == n && (!n || !memcmp(one.data(), dec.data(), n * sizeof one[0])));
        for (uint32_t k = 0; k < n; ++k) {
            CHECK(enc[k].spi == dec[k].spi && !enc[k].pad[0] && !enc[k].pad[1] && !enc[k].pad[2]);
            const fcgpu_espaes_sa *src = nullptr;
            for (const auto &s : sa)
                if (s.spi == dec[k].spi) src = &s;
            CHECK(src);
            fcaes::dec_round_keys(src->enc_key, dk);
            CHECK(!memcmp(dk, dec[k].rk, sizeof dk) && !memcmp(enc[k].rk, src->enc_key, 16));
            uint8_t p[16], c[16], d[16];
            for (auto &b : p) b = (uint8_t)rng();
            fcaes::encrypt_block(enc[k].rk, p, c);
            fcaes::decrypt_block(dec[k].rk, c, d);
            CHECK(!memcmp(p, d, 16) && memcmp(p, c, 16));
        }
    }
    printf("aes_enc_key_check ok\n");
    return 0;
}
