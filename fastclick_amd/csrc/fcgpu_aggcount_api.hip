// fcgpu_aggcount_api.hip -- AggregateCounter on the device: the control calls
// (fcgpu_aggcount_configure ... fcgpu_aggcount_read) and the launches of the
// post-pass k_aggcount behind k_rx (process_one) and of the dump k_aggdump
// (fcgpu_aggcount.hh).
#include "fcgpu_internal.hh"
#include "fcgpu_aggcount.hh"

using namespace fcgpu;
using namespace fcgpu_rt;

static_assert(kAgcMaxCapacity == FCGPU_AGGCOUNT_MAX_CAPACITY, "capacity limit is part of the ABI");
static_assert(sizeof(fcgpu_aggcount_rec) == sizeof(uint4), "k_aggdump writes records as uint4");
static_assert(sizeof(fcgpu_anno) == 16 && offsetof(fcgpu_anno, length) == 4 && offsetof(fcgpu_anno, nh) == 8,
              "k_aggcount reads length and nh from words 1 and 2 of an annotation");

namespace fcgpu_rt {

void aggcount_free(fcgpu_ctx *c) {
    for (void *p : {(void *)c->agc_tab, (void *)c->agc_state, (void *)c->agc_verdict, (void *)c->agc_hash,
                    (void *)c->agc_anno})
        hipFree(p);
    c->agc_tab = c->agc_state = nullptr;
    c->agc_verdict = nullptr;
    c->agc_hash = nullptr;
    c->agc_anno = nullptr;
    c->agc_slots = 0;
    c->agc_conf = fcgpu_aggcount_config{};
    c->agc_frozen = false;
}

// Up to 8 workgroups per CU, each looping over tiles, so the totals cost at
// most that many adds per batch.
hipError_t launch_aggcount(const fcgpu_ctx *c, const uint16_t *verdict, const uint32_t *hash, const fcgpu_anno *anno,
                           uint32_t n, hipStream_t s) {
    const uint32_t mode = c->agc_conf.bytes ? (c->agc_conf.ip_bytes ? 2u : 1u) : 0u;
    if (!c->agc_tab || !verdict || !hash || (mode && !anno) || n > c->max_batch) return hipErrorInvalidValue;
    AgcArgs a;
    a.verdict = verdict;
    a.hash = hash;
    a.anno = reinterpret_cast<const uint32_t *>(anno);
    a.n = n;
    a.ntiles = (n + kTile - 1) / kTile;
    a.mask = c->agc_conf.mask;
    a.mode = mode;
    a.tab = c->agc_tab;
    a.state = c->agc_state;
    a.shift = 32u - (uint32_t)__builtin_ctz(c->agc_slots);
    a.slot_mask = c->agc_slots - 1;
    a.capacity = c->agc_conf.capacity;
    const uint32_t grid = std::min(a.ntiles, std::max(1u, c->ncu) * 8u);
    if (!grid) return hipSuccess;
    if (c->agc_frozen) hipLaunchKernelGGL(k_aggcount<true>, dim3(grid), dim3(kTile), 0, s, a);
    else hipLaunchKernelGGL(k_aggcount<false>, dim3(grid), dim3(kTile), 0, s, a);
    return hipGetLastError();
}

static int aggcount_state(fcgpu_ctx *c, unsigned long long *w) {
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, hipMemcpy(w, c->agc_state, sizeof(unsigned long long) * kAgcStateWords, hipMemcpyDeviceToHost));
    return FCGPU_OK;
}

}  // namespace fcgpu_rt

extern "C" {

int fcgpu_aggcount_configure(fcgpu_ctx *c, const fcgpu_aggcount_config *cfg) {
    if (!c || !cfg) return FCGPU_EINVAL;
    if (agg_queued(c))
        return fail(c, FCGPU_EINVAL, "fcgpu_aggcount_configure: a queued span submission is not waited for");
    if (cfg->capacity > FCGPU_AGGCOUNT_MAX_CAPACITY)
        return fail(c, FCGPU_EINVAL, "fcgpu_aggcount_configure: capacity above FCGPU_AGGCOUNT_MAX_CAPACITY (1 << 24)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    if (!cfg->capacity) {
        aggcount_free(c);
        return FCGPU_OK;
    }
    if (!c->ncu) {
        int cu = 0;
        HIPCHK(c, hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, c->device));
        c->ncu = (uint32_t)std::max(cu, 1);
    }
    uint32_t slots = 2;
    while (slots < 2 * cfg->capacity) slots <<= 1;
    // made before the old counter is freed: a failure leaves it intact
    unsigned long long *tab = nullptr, *state = nullptr;
    uint16_t *v = nullptr;
    uint32_t *h = nullptr;
    fcgpu_anno *an = nullptr;
    const size_t nb = std::max(c->max_batch, 1u);
    if (int rc = alloc_or_fail(c, "fcgpu_aggcount_configure",
                               {dev_buf(tab, sizeof(unsigned long long) * 2 * (size_t)slots, true),
                                dev_buf(state, sizeof(unsigned long long) * kAgcStateWords, true),
                                dev_buf(v, sizeof(uint16_t) * nb), dev_buf(h, sizeof(uint32_t) * nb),
                                dev_buf(an, sizeof(fcgpu_anno) * nb)}))
        return rc;
    aggcount_free(c);
    c->agc_tab = tab;
    c->agc_state = state;
    c->agc_verdict = v;
    c->agc_hash = h;
    c->agc_anno = an;
    c->agc_slots = slots;
    c->agc_conf = *cfg;
    c->agc_conf.bytes = cfg->bytes ? 1u : 0u;
    c->agc_conf.ip_bytes = cfg->ip_bytes ? 1u : 0u;
    if (!c->agc_conf.mask) c->agc_conf.mask = 0xffffffffu;
    return FCGPU_OK;
}

int fcgpu_aggcount_freeze(fcgpu_ctx *c, int frozen) {
    if (!c) return FCGPU_EINVAL;
    if (!c->agc_tab) return fail(c, FCGPU_EINVAL, "fcgpu_aggcount_freeze: the counter is not enabled");
    c->agc_frozen = frozen != 0;     // the next batch's launch takes it
    return FCGPU_OK;
}

int fcgpu_aggcount_reset(fcgpu_ctx *c) {
    if (!c) return FCGPU_EINVAL;
    if (agg_queued(c)) return fail(c, FCGPU_EINVAL, "fcgpu_aggcount_reset: a queued span submission is not waited for");
    if (!c->agc_tab) return FCGPU_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    HIPCHK(c, memset_sync(c->agc_tab, 0, sizeof(unsigned long long) * 2 * (size_t)c->agc_slots));
    HIPCHK(c, memset_sync(c->agc_state, 0, sizeof(unsigned long long) * kAgcStateWords));
    return FCGPU_OK;
}

int fcgpu_aggcount_stats(fcgpu_ctx *c, fcgpu_aggcount_stat *st) {
    if (!c || !st) return FCGPU_EINVAL;
    *st = fcgpu_aggcount_stat{};
    if (!c->agc_tab) return FCGPU_OK;
    unsigned long long w[kAgcStateWords];
    if (int rc = aggcount_state(c, w)) return rc;
    st->capacity = c->agc_conf.capacity;
    st->nagg = (uint32_t)std::min<unsigned long long>(w[kAgcNagg], c->agc_conf.capacity);   // tickets past it were refused
    st->nnz = (uint32_t)w[kAgcNnz];
    st->frozen = c->agc_frozen ? 1u : 0u;
    st->count = w[kAgcCount];
    st->seen = w[kAgcSeen];
    st->uncounted = w[kAgcUncounted];
    return FCGPU_OK;
}

int fcgpu_aggcount_read(fcgpu_ctx *c, fcgpu_aggcount_rec *h_out, uint32_t max, uint32_t *n) {
    if (!c || !n || (max && !h_out)) return FCGPU_EINVAL;
    *n = 0;
    if (!c->agc_tab) return FCGPU_OK;
    unsigned long long w[kAgcStateWords];
    if (int rc = aggcount_state(c, w)) return rc;
    const uint32_t nnz = (uint32_t)w[kAgcNnz];
    *n = nnz;
    if (!nnz || !max) return FCGPU_OK;
    // the dump is unordered: all nnz records come to the host, are sorted
    // there and the first max go to the caller (a control-path read; the
    // reference walks its radix tree)
    fcgpu_aggcount_rec *d_rec = nullptr;
    if (int rc = alloc_or_fail(c, "fcgpu_aggcount_read", {dev_buf(d_rec, sizeof(fcgpu_aggcount_rec) * (size_t)nnz)}))
        return rc;
    std::vector<fcgpu_aggcount_rec> rec(nnz);
    unsigned long long found = 0;
    hipError_t e = memset_sync(c->agc_state + kAgcDumped, 0, sizeof(unsigned long long));
    if (e == hipSuccess) {
        const uint32_t grid = std::min((c->agc_slots + kTile - 1) / kTile, std::max(1u, c->ncu) * 8u);
        hipLaunchKernelGGL(k_aggdump, dim3(grid), dim3(kTile), 0, nullptr, c->agc_tab, c->agc_slots,
                           reinterpret_cast<uint4 *>(d_rec), nnz, c->agc_state);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(&found, c->agc_state + kAgcDumped, sizeof found, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(rec.data(), d_rec, sizeof(fcgpu_aggcount_rec) * (size_t)nnz, hipMemcpyDeviceToHost);
    (void)hipFree(d_rec);
    if (e != hipSuccess) return fail(c, FCGPU_ERUNTIME, std::string("fcgpu_aggcount_read: ") + hipGetErrorString(e));
    if (found != nnz) return fail(c, FCGPU_ERUNTIME, "fcgpu_aggcount_read: the dump and nnz disagree");
    std::sort(rec.begin(), rec.end(),
              [](const fcgpu_aggcount_rec &x, const fcgpu_aggcount_rec &y) { return x.agg < y.agg; });
    memcpy(h_out, rec.data(), sizeof(fcgpu_aggcount_rec) * std::min(max, nnz));
    return FCGPU_OK;
}

}  // extern "C"
