// esp_sa_check.cc -- host-code sanitizer run of host/esp_sa.hh (TEST
// INFRASTRUCTURE, CPU only; built with -fsanitize=address,undefined by
// tests/test_espauth_host.py). Midstate-based HMAC-SHA1 against RFC 2202 test
// cases 1-3 and 6 (case 6's 80-byte key is hashed first, RFC 2104, so every
// key handed to hmac_midstates is <= 64 B), the SA image of seeded random
// tables (sorted, midstates reproduce the direct HMAC) and the refusals.
// Prints "esp_sa_check ok" and exits 0, or reports the failed check.
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include "../fastclick_amd/csrc/host/esp_sa.hh"

#define CHECK(c)                                                                       \
    do {                                                                               \
        if (!(c)) {                                                                    \
            fprintf(stderr, "esp_sa_check: failed at %s:%d: %s\n", __FILE__, __LINE__, #c); \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)

static std::vector<uint8_t> hmac(std::vector<uint8_t> key, const std::vector<uint8_t> &msg) {
    if (key.size() > 64) {
        std::vector<uint8_t> d(20);
        fcesp::sha1(key.data(), key.size(), d.data());
        key = d;
    }
    uint32_t in[5], out[5];
    CHECK(fcesp::hmac_midstates(key.data(), key.size(), in, out));
    std::vector<uint8_t> mac(20);
    fcesp::hmac_from_midstates(in, out, msg.data(), msg.size(), mac.data());
    return mac;
}

static std::vector<uint8_t> hex(const char *s) {
    std::vector<uint8_t> v;
    for (; s[0] && s[1]; s += 2) v.push_back((uint8_t)strtoul(std::string(s, 2).c_str(), nullptr, 16));
    return v;
}
static std::vector<uint8_t> str(const char *s) { return std::vector<uint8_t>(s, s + strlen(s)); }

int main() {
    // RFC 2202 section 3
    CHECK(hmac(std::vector<uint8_t>(20, 0x0b), str("Hi There")) == hex("b617318655057264e28bc0b6fb378c8ef146be00"));
    CHECK(hmac(str("Jefe"), str("what do ya want for nothing?")) == hex("effcdf6ae5eb2fa2d27416d5f184df9c259a7c79"));
    CHECK(hmac(std::vector<uint8_t>(20, 0xaa), std::vector<uint8_t>(50, 0xdd)) ==
          hex("125d7342b9ac11cd91a39af48aa17b4f63f175d3"));
    CHECK(hmac(std::vector<uint8_t>(80, 0xaa), str("Test Using Larger Than Block-Size Key - Hash Key First")) ==
          hex("aa4ae5e15272d00e95705637ce8a3b55ed402112"));
    uint32_t in[5], out[5];
    uint8_t big[65] = {0};
    CHECK(!fcesp::hmac_midstates(big, 65, in, out));

    std::mt19937 rng(12345);
    std::vector<fcesp::SaDev> im;
    std::string err;
    for (uint32_t n : {0u, 1u, 2u, 341u, 342u, 5000u}) {
        std::vector<fcgpu_esp_sa> sa(n);
        for (uint32_t k = 0; k < n; ++k) {
            sa[k].spi = 1 + k * 7919u % 100003u;      // distinct, unsorted
            for (auto &b : sa[k].auth_key) b = (uint8_t)rng();
        }
        CHECK(fcesp::build(sa.data(), n, im, err) == FCGPU_OK && im.size() == n);
        for (uint32_t k = 0; k < n; ++k) {
            CHECK(k == 0 || im[k - 1].spi < im[k].spi);
            const fcgpu_esp_sa *src = nullptr;
            for (const auto &s : sa)
                if (s.spi == im[k].spi) src = &s;
            CHECK(src);
            // messages around the one- and two-block paddings
            for (size_t len : {0u, 16u, 54u, 55u, 56u, 63u, 64u, 65u, 119u, 120u, 1454u}) {
                if (k % 97 && len > 64) continue;
                std::vector<uint8_t> msg(len);
                for (auto &b : msg) b = (uint8_t)rng();
                uint8_t mac[20];
                fcesp::hmac_from_midstates(im[k].inner, im[k].outer, msg.data(), len, mac);
                CHECK(hmac(std::vector<uint8_t>(src->auth_key, src->auth_key + 16), msg) ==
                      std::vector<uint8_t>(mac, mac + 20));
            }
        }
        // refusals leave the image as it is
        if (n >= 2) {
            const std::vector<fcesp::SaDev> keep = im;
            std::vector<fcgpu_esp_sa> bad = sa;
            bad[n - 1].spi = bad[0].spi;
            CHECK(fcesp::build(bad.data(), n, im, err) == FCGPU_EINVAL && err.find("duplicate") != std::string::npos);
            bad = sa;
            bad[n / 2].spi = 0;
            CHECK(fcesp::build(bad.data(), n, im, err) == FCGPU_EINVAL && err.find("SPI 0") != std::string::npos);
            CHECK(im.size() == keep.size() && !memcmp(im.data(), keep.data(), keep.size() * sizeof keep[0]));
        }
    }
    std::vector<fcgpu_esp_sa> many(fcesp::kMaxSas + 1);
    for (uint32_t k = 0; k < many.size(); ++k) many[k].spi = k + 1;
    CHECK(fcesp::build(many.data(), (uint32_t)many.size(), im, err) == FCGPU_EINVAL);
    CHECK(fcesp::build(many.data(), fcesp::kMaxSas, im, err) == FCGPU_OK && im.size() == fcesp::kMaxSas);
    printf("esp_sa_check ok\n");
    return 0;
}
