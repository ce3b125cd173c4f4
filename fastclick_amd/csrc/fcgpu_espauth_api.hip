// fcgpu_espauth_api.hip -- ESP authentication (IPsecAuthHMACSHA1) on the
// device: the control calls (fcgpu_espauth_set_sas ... fcgpu_espauth_reset)
// and the launch of the post-pass k_espauth behind k_rx (process_one)
// (fcgpu_espauth.hh, host/esp_sa.hh).
#include "fcgpu_internal.hh"
#include "fcgpu_espauth.hh"
#include "host/esp_sa.hh"

using namespace fcgpu;
using namespace fcgpu_rt;

static_assert(fcesp::kMaxSas == FCGPU_ESPAUTH_MAX_SAS, "the SA limit is part of the ABI");
static_assert(sizeof(fcesp::SaDev) == kEspSaWords * sizeof(uint32_t), "k_espauth reads 12 words per SA");
static_assert(sizeof(fcgpu_esp_rec) == sizeof(uint4) && offsetof(fcgpu_esp_rec, icv) == 4,
              "k_espauth writes records as uint4 {status, icv words}");
static_assert(sizeof(fcgpu_espauth_stat) <= kEspStatWords * sizeof(unsigned long long) &&
                  offsetof(fcgpu_espauth_stat, not_esp) == 4 * sizeof(uint64_t),
              "k_espauth's counters are in the order of fcgpu_espauth_stat");
static_assert(sizeof(fcgpu_anno) == 16 && offsetof(fcgpu_anno, length) == 4 && offsetof(fcgpu_anno, nh) == 8 &&
                  offsetof(fcgpu_anno, ipver) == 13,
              "k_espauth reads length, nh and ipver from words 1, 2 and 3 of an annotation");
static_assert(FCGPU_ESP_OK == 1 && FCGPU_ESP_BAD == 2 && FCGPU_ESP_NO_SA == 3 && FCGPU_ESP_SHORT == 4, "status codes");

namespace fcgpu_rt {

void espauth_free(fcgpu_ctx *c) {
    for (void *p : {(void *)c->esp_sa, (void *)c->esp_rec, (void *)c->esp_stat, (void *)c->esp_verdict,
                    (void *)c->esp_anno})
        hipFree(p);
    c->esp_sa = nullptr;
    c->esp_rec = nullptr;
    c->esp_stat = nullptr;
    c->esp_verdict = nullptr;
    c->esp_anno = nullptr;
    c->esp_nsa = 0;
}

// Workgroups per CU: the kernel holds 36.3 KB of static LDS (segment buffers
// and packet slots) and, with the SA image staged, up to 16 KB more: three
// fit a CU's 160 KB with the image, four without; each loops over tiles.
hipError_t launch_espauth(const fcgpu_ctx *c, const uint8_t *arena, const uint32_t *desc, const uint16_t *verdict,
                          const fcgpu_anno *anno, uint32_t n, hipStream_t s) {
    if (!c->esp_sa || !c->esp_nsa || !arena || !desc || !verdict || !anno || n > c->max_batch)
        return hipErrorInvalidValue;
    if (!n) return hipSuccess;
    EspArgs a;
    a.arena = arena;              // FCGPU_ESP_SEAL writes the digests into it (include/fastclick_gpu.h)
    a.desc = reinterpret_cast<const uint2 *>(desc);
    a.verdict = verdict;
    a.anno = reinterpret_cast<const uint32_t *>(anno);
    a.n = n;
    a.ntiles = (n + kTile - 1) / kTile;
    a.mode = c->esp_mode;
    a.sa = c->esp_sa;
    a.nsa = c->esp_nsa;
    const size_t image = (size_t)c->esp_nsa * sizeof(fcesp::SaDev);
    a.sa_lds = image <= kEspLdsImage ? 1u : 0u;
    a.rec = c->esp_rec;
    a.stat = c->esp_stat;
    const uint32_t grid = std::min(a.ntiles, std::max(1u, c->ncu) * (a.sa_lds ? 3u : 4u));
    const size_t dyn = a.sa_lds ? image : 0;
    if (c->esp_order) hipLaunchKernelGGL(k_espauth<true>, dim3(grid), dim3(kTile), dyn, s, a);
    else hipLaunchKernelGGL(k_espauth<false>, dim3(grid), dim3(kTile), dyn, s, a);
    return hipGetLastError();
}

}  // namespace fcgpu_rt

extern "C" {

int fcgpu_espauth_set_sas(fcgpu_ctx *c, const fcgpu_esp_sa *sas, uint32_t n) {
    if (!c || (n && !sas)) return FCGPU_EINVAL;
    if (agg_queued(c)) return fail(c, FCGPU_EINVAL, "fcgpu_espauth_set_sas: a queued span submission is not waited for");
    std::vector<fcesp::SaDev> im;
    std::string err;
    if (fcesp::build(sas, n, im, err) != FCGPU_OK) return fail(c, FCGPU_EINVAL, "fcgpu_espauth_set_sas: " + err);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    if (!n) {
        espauth_free(c);
        return FCGPU_OK;
    }
    if (!c->ncu) {
        int cu = 0;
        HIPCHK(c, hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, c->device));
        c->ncu = (uint32_t)std::max(cu, 1);
    }
    // made before the old table is freed: a failure leaves it installed
    uint32_t *sa = nullptr;
    uint4 *rec = nullptr;
    unsigned long long *stat = nullptr;
    uint16_t *v = nullptr;
    fcgpu_anno *an = nullptr;
    const size_t nb = std::max(c->max_batch, 1u), bytes = im.size() * sizeof(fcesp::SaDev);
    if (int rc = alloc_or_fail(c, "fcgpu_espauth_set_sas",
                               {dev_buf(sa, bytes), dev_buf(rec, sizeof(uint4) * nb, true),
                                dev_buf(stat, sizeof(unsigned long long) * kEspStatWords, true),
                                dev_buf(v, sizeof(uint16_t) * nb), dev_buf(an, sizeof(fcgpu_anno) * nb)}))
        return rc;
    if (hipError_t e = hipMemcpy(sa, im.data(), bytes, hipMemcpyHostToDevice)) {
        for (void *p : {(void *)sa, (void *)rec, (void *)stat, (void *)v, (void *)an}) hipFree(p);
        return fail(c, FCGPU_ERUNTIME, std::string("fcgpu_espauth_set_sas: ") + hipGetErrorString(e));
    }
    espauth_free(c);
    c->esp_sa = sa;
    c->esp_nsa = n;
    c->esp_rec = rec;
    c->esp_stat = stat;
    c->esp_verdict = v;
    c->esp_anno = an;
    // tuning knob: FCGPU_ESPAUTH_ORDER=0 leaves every tile in arrival order
    const char *e = getenv("FCGPU_ESPAUTH_ORDER");
    c->esp_order = !(e && e[0] == '0');
    return FCGPU_OK;
}

int fcgpu_espauth_configure(fcgpu_ctx *c, const fcgpu_espauth_config *cfg) {
    if (!c || !cfg) return FCGPU_EINVAL;
    if (cfg->mode > FCGPU_ESP_SEAL) return fail(c, FCGPU_EINVAL, "fcgpu_espauth_configure: bad mode");
    c->esp_mode = cfg->mode;      // the next batch's launch takes it
    return FCGPU_OK;
}

int fcgpu_espauth_records(fcgpu_ctx *c, const fcgpu_esp_rec **d_rec) {
    if (!c || !d_rec) return FCGPU_EINVAL;
    *d_rec = reinterpret_cast<const fcgpu_esp_rec *>(c->esp_rec);
    return FCGPU_OK;
}

int fcgpu_espauth_stats(fcgpu_ctx *c, fcgpu_espauth_stat *st) {
    if (!c || !st) return FCGPU_EINVAL;
    *st = fcgpu_espauth_stat{};
    if (!c->esp_sa) return FCGPU_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(st, c->esp_stat, sizeof *st, hipMemcpyDeviceToHost));
    return FCGPU_OK;
}

int fcgpu_espauth_reset(fcgpu_ctx *c) {
    if (!c) return FCGPU_EINVAL;
    if (agg_queued(c)) return fail(c, FCGPU_EINVAL, "fcgpu_espauth_reset: a queued span submission is not waited for");
    if (!c->esp_sa) return FCGPU_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, memset_sync(c->esp_stat, 0, sizeof(unsigned long long) * kEspStatWords));
    return FCGPU_OK;
}

}  // extern "C"
