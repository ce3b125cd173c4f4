// fcgpu_espaes_api.hip -- ESP decryption and encryption (IPsecAES(0) / (1)) on
// the device: the control calls (fcgpu_espaes_set_sas ... fcgpu_espaes_reset)
// and the launch of the post-pass behind k_rx (process_one): k_espaes in front
// of k_espauth, or k_espenc behind it (fcgpu_espaes.hh, fcgpu_espenc.hh,
// host/aes_key.hh).
#include "fcgpu_internal.hh"
#include "fcgpu_espaes.hh"
#include "fcgpu_espenc.hh"

using namespace fcgpu;
using namespace fcgpu_rt;

static_assert(fcaes::kMaxSas == FCGPU_ESPAES_MAX_SAS, "the SA limit is part of the ABI");
static_assert(sizeof(fcaes::SaDev) == kAesSaWords * sizeof(uint32_t) && offsetof(fcaes::SaDev, rk) == 4,
              "k_espaes reads 48 words per SA, the round keys from word 1");
static_assert(sizeof(fcgpu_espaes_stat) == kAesStatWords * sizeof(unsigned long long) &&
                  offsetof(fcgpu_espaes_stat, blocks) == 5 * sizeof(uint64_t),
              "k_espaes's counters are in the order of fcgpu_espaes_stat");
static_assert(sizeof(fcgpu_anno) == 16 && offsetof(fcgpu_anno, length) == 4 && offsetof(fcgpu_anno, nh) == 8 &&
                  offsetof(fcgpu_anno, ipver) == 13,
              "k_espaes reads length, nh and ipver from words 1, 2 and 3 of an annotation");
static_assert(FCGPU_ESP_OK == 1 && FCGPU_ESP_NO_SA == 3 && FCGPU_ESP_SHORT == 4 && FCGPU_ESP_UNALIGNED == 5, "status codes");

// The device buffer aes_sa: Td0 (256 words), the inverse S-box (64 words),
// the decryption records, then the encryption records and Te0 (256 words).
constexpr size_t kAesTabWords = 256 + 64;

namespace fcgpu_rt {

void espaes_free(fcgpu_ctx *c) {
    for (void *p : {(void *)c->aes_sa, (void *)c->aes_status, (void *)c->aes_stat, (void *)c->aes_verdict,
                    (void *)c->aes_anno})
        hipFree(p);
    c->aes_sa = nullptr;
    c->aes_status = nullptr;
    c->aes_stat = nullptr;
    c->aes_verdict = nullptr;
    c->aes_anno = nullptr;
    c->aes_nsa = 0;
}

template <int NTAB, int REPL> static void launch_variant(uint32_t grid, size_t dyn, hipStream_t s, const AesArgs &a) {
    hipLaunchKernelGGL((k_espaes<NTAB, REPL>), dim3(grid), dim3(kTile), dyn, s, a);
}

// Workgroups per CU: the kernel holds the tables (NTAB x REPL KB and REPL x
// 256 B), 4.2 KB of tile arrays and, with the SA image staged, up to 16 KB
// more: four workgroups a CU, 16 waves, each looping over tiles. A batch with
// fewer than that many 256-packet tiles is cut into smaller tiles (down to 32
// packets: a 1500-byte frame has 91 blocks, so 32 of them still fill 11
// passes of 256 lanes).
//
// k_espenc (FCGPU_ESPAES_ENCRYPT) serves 16 packets a wave, so a 256-packet
// tile is 16 groups for 4 waves. It holds 4.4 KB of static LDS and up to 16 KB
// of image; 102 SGPRs allow 7 waves a SIMD. The launch asks for kEncWgPerCu =
// 7 workgroups a CU (the chain of dependent rounds wants waves to hide behind)
// and cuts the tiles of a small batch down to kEncMinTile = 64 packets, one
// group per wave: 43,690 x 1500 B is 683 workgroups, 2,731 waves.
static hipError_t launch_espenc(const fcgpu_ctx *c, uint8_t *arena, const uint32_t *desc, const uint16_t *verdict,
                                const fcgpu_anno *anno, uint32_t n, hipStream_t s) {
    EncArgs a;
    a.arena = arena;                            // encrypted in place (include/fastclick_gpu.h)
    a.desc = reinterpret_cast<const uint2 *>(desc);
    a.verdict = verdict;
    a.anno = reinterpret_cast<const uint32_t *>(anno);
    a.n = n;
    const uint32_t slots = std::max(1u, c->ncu) * kEncWgPerCu;
    a.tpk = c->aes_tile ? c->aes_tile : (uint32_t)kTile;
    while (!c->aes_tile && a.tpk > kEncMinTile && (n + a.tpk - 1) / a.tpk < slots) a.tpk >>= 1;
    a.ntiles = (n + a.tpk - 1) / a.tpk;
    const size_t image = (size_t)c->aes_nsa * sizeof(fcaes::SaDev);
    a.sa = c->aes_sa + kAesTabWords + (size_t)c->aes_nsa * kAesSaWords;
    a.te0 = a.sa + (size_t)c->aes_nsa * kAesSaWords;
    a.nsa = c->aes_nsa;
    a.sa_lds = image <= kAesLdsImage ? 1u : 0u;
    a.status = c->aes_status;
    a.stat = c->aes_stat;
    const uint32_t grid = std::min(a.ntiles, slots);
    const size_t dyn = a.sa_lds ? image : 0;
    if (c->aes_order) hipLaunchKernelGGL(k_espenc<true>, dim3(grid), dim3(kTile), dyn, s, a);
    else hipLaunchKernelGGL(k_espenc<false>, dim3(grid), dim3(kTile), dyn, s, a);
    return hipGetLastError();
}

hipError_t launch_espaes(const fcgpu_ctx *c, const uint8_t *arena, const uint32_t *desc, const uint16_t *verdict,
                         const fcgpu_anno *anno, uint32_t n, hipStream_t s) {
    if (!c->aes_sa || !c->aes_nsa || !arena || !desc || !verdict || !anno || n > c->max_batch)
        return hipErrorInvalidValue;
    if (!n) return hipSuccess;
    if (c->aes_mode == FCGPU_ESPAES_ENCRYPT) return launch_espenc(c, const_cast<uint8_t *>(arena), desc, verdict, anno, n, s);
    AesArgs a;
    a.arena = const_cast<uint8_t *>(arena);     // decrypted in place (include/fastclick_gpu.h)
    a.desc = reinterpret_cast<const uint2 *>(desc);
    a.verdict = verdict;
    a.anno = reinterpret_cast<const uint32_t *>(anno);
    a.n = n;
    const uint32_t slots = std::max(1u, c->ncu) * 4u;
    a.tpk = c->aes_tile ? c->aes_tile : (uint32_t)kTile;
    while (!c->aes_tile && a.tpk > 32 && (n + a.tpk - 1) / a.tpk < slots) a.tpk >>= 1;
    a.ntiles = (n + a.tpk - 1) / a.tpk;
    a.td0 = c->aes_sa;
    a.isb = c->aes_sa + 256;
    a.sa = c->aes_sa + kAesTabWords;
    a.nsa = c->aes_nsa;
    const size_t image = (size_t)c->aes_nsa * sizeof(fcaes::SaDev);
    a.sa_lds = image <= kAesLdsImage ? 1u : 0u;
    a.status = c->aes_status;
    a.stat = c->aes_stat;
    const uint32_t grid = std::min(a.ntiles, slots);
    const size_t dyn = a.sa_lds ? image : 0;
    switch (c->aes_ntab * 8 + c->aes_repl) {
    case 1 * 8 + 1: launch_variant<1, 1>(grid, dyn, s, a); break;
    case 1 * 8 + 2: launch_variant<1, 2>(grid, dyn, s, a); break;
    case 1 * 8 + 4: launch_variant<1, 4>(grid, dyn, s, a); break;
    case 4 * 8 + 1: launch_variant<4, 1>(grid, dyn, s, a); break;
    case 4 * 8 + 2: launch_variant<4, 2>(grid, dyn, s, a); break;
    case 4 * 8 + 4: launch_variant<4, 4>(grid, dyn, s, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace fcgpu_rt

extern "C" {

int fcgpu_espaes_set_sas(fcgpu_ctx *c, const fcgpu_espaes_sa *sas, uint32_t n) {
    if (!c || (n && !sas)) return FCGPU_EINVAL;
    if (agg_queued(c)) return fail(c, FCGPU_EINVAL, "fcgpu_espaes_set_sas: a queued span submission is not waited for");
    std::vector<fcaes::SaDev> im, enc;
    std::string err;
    if (fcaes::build(sas, n, im, err, &enc) != FCGPU_OK) return fail(c, FCGPU_EINVAL, "fcgpu_espaes_set_sas: " + err);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    if (!n) {
        espaes_free(c);
        return FCGPU_OK;
    }
    if (!c->ncu) {
        int cu = 0;
        HIPCHK(c, hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, c->device));
        c->ncu = (uint32_t)std::max(cu, 1);
    }
    std::vector<uint32_t> host(kAesTabWords + 2 * im.size() * kAesSaWords + 256);
    memcpy(host.data(), fcaes::kTables.td0, 1024);
    memcpy(host.data() + 256, fcaes::kTables.isbox, 256);
    memcpy(host.data() + kAesTabWords, im.data(), im.size() * sizeof(fcaes::SaDev));
    memcpy(host.data() + kAesTabWords + im.size() * kAesSaWords, enc.data(), enc.size() * sizeof(fcaes::SaDev));
    memcpy(host.data() + kAesTabWords + 2 * im.size() * kAesSaWords, fcaes::kTables.te0, 1024);
    // made before the old table is freed: a failure leaves it installed
    uint32_t *sa = nullptr;
    uint8_t *status = nullptr;
    unsigned long long *stat = nullptr;
    uint16_t *v = nullptr;
    fcgpu_anno *an = nullptr;
    const size_t nb = std::max(c->max_batch, 1u), bytes = host.size() * sizeof(uint32_t);
    if (int rc = alloc_or_fail(c, "fcgpu_espaes_set_sas",
                               {dev_buf(sa, bytes), dev_buf(status, nb, true),
                                dev_buf(stat, sizeof(unsigned long long) * kAesStatWords, true),
                                dev_buf(v, sizeof(uint16_t) * nb), dev_buf(an, sizeof(fcgpu_anno) * nb)}))
        return rc;
    if (hipError_t e = hipMemcpy(sa, host.data(), bytes, hipMemcpyHostToDevice)) {
        for (void *p : {(void *)sa, (void *)status, (void *)stat, (void *)v, (void *)an}) hipFree(p);
        return fail(c, FCGPU_ERUNTIME, std::string("fcgpu_espaes_set_sas: ") + hipGetErrorString(e));
    }
    espaes_free(c);
    c->aes_sa = sa;
    c->aes_nsa = n;
    c->aes_status = status;
    c->aes_stat = stat;
    c->aes_verdict = v;
    c->aes_anno = an;
    // tuning knobs: FCGPU_ESPAES_TABLES = 1 | 4 tables in
    // LDS, FCGPU_ESPAES_REPLICAS = 1 | 2 | 4 copies of them, FCGPU_ESPAES_TILE
    // = 32 | 64 | 128 | 256 packets per tile whatever the batch's size (both
    // kernels); FCGPU_ESPENC_ORDER=0 leaves k_espenc's tiles in arrival order
    // 
    const char *et = getenv("FCGPU_ESPAES_TABLES"), *er = getenv("FCGPU_ESPAES_REPLICAS"), *ep = getenv("FCGPU_ESPAES_TILE");
    const char *eo = getenv("FCGPU_ESPENC_ORDER");
    c->aes_order = !(eo && eo[0] == '0');
    const uint32_t tp = ep ? (uint32_t)atoi(ep) : 0u;
    c->aes_tile = tp == 32 || tp == 64 || tp == 128 || tp == 256 ? tp : 0u;
    c->aes_ntab = et && et[0] == '1' ? 1 : et && et[0] == '4' ? 4 : kAesDefaultTables;
    c->aes_repl = er && (er[0] == '1' || er[0] == '2' || er[0] == '4') ? (uint32_t)(er[0] - '0') : kAesDefaultReplicas;
    return FCGPU_OK;
}

int fcgpu_espaes_configure(fcgpu_ctx *c, const fcgpu_espaes_config *cfg) {
    if (!c || !cfg) return FCGPU_EINVAL;
    if (cfg->mode > FCGPU_ESPAES_ENCRYPT) return fail(c, FCGPU_EINVAL, "fcgpu_espaes_configure: bad mode");
    c->aes_mode = cfg->mode;      // the next batch's launch takes it
    return FCGPU_OK;
}

int fcgpu_espaes_status(fcgpu_ctx *c, const uint8_t **d_status) {
    if (!c || !d_status) return FCGPU_EINVAL;
    *d_status = c->aes_status;
    return FCGPU_OK;
}

int fcgpu_espaes_stats(fcgpu_ctx *c, fcgpu_espaes_stat *st) {
    if (!c || !st) return FCGPU_EINVAL;
    *st = fcgpu_espaes_stat{};
    if (!c->aes_sa) return FCGPU_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(st, c->aes_stat, sizeof *st, hipMemcpyDeviceToHost));
    return FCGPU_OK;
}

int fcgpu_espaes_reset(fcgpu_ctx *c) {
    if (!c) return FCGPU_EINVAL;
    if (agg_queued(c)) return fail(c, FCGPU_EINVAL, "fcgpu_espaes_reset: a queued span submission is not waited for");
    if (!c->aes_sa) return FCGPU_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, memset_sync(c->aes_stat, 0, sizeof(unsigned long long) * kAesStatWords));
    return FCGPU_OK;
}

}  // extern "C"
