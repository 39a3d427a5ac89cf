// sgdmp_api.hip -- the C ABI of include/ccnet_sgdmp.h (libccnet_sgdmp.so): the chunk plan, the table checks and the launches.
// The launches go on the caller's stream and nothing waits for the device.
#include "ccnet_sgdmp.h"

#include "sgdmp_kernels.hpp"

#define CCNET_ERROR_PREFIX "ccnet_sgdmp: "
#include "../csrc_common/ccnet_host.hpp"

namespace {

constexpr int64_t kMaxNumel = 0x7fffffffLL;

int64_t chunks_of(int64_t numel) { return (numel + CCNET_SGD_CHUNK - 1) / CCNET_SGD_CHUNK; }

}  // namespace

extern "C" {

__attribute__((visibility("default"))) int ccnet_sgdmp_version(void) { return CCNET_SGDMP_VERSION; }
__attribute__((visibility("default"))) const char *ccnet_sgdmp_arch(void) { return "gfx950"; }
__attribute__((visibility("default"))) const char *ccnet_sgdmp_last_error_string(void) { return g_err; }

__attribute__((visibility("default"))) int ccnet_sgdmp_plan(const int64_t *numel, int n_tensors, int32_t *chunks, int64_t capacity,
                                                            int64_t *n_chunks) {
    if (!numel || !n_chunks) return fail(-2, "plan: NULL numel or n_chunks");
    if (n_tensors < 1 || n_tensors > CCNET_SGD_MAX_TENSORS)
        return fail(-1, "plan: %d tensors, outside 1..%d", n_tensors, CCNET_SGD_MAX_TENSORS);
    int64_t total = 0;
    for (int t = 0; t < n_tensors; ++t) {
        if (numel[t] < 1 || numel[t] > kMaxNumel)
            return fail(-3, "plan: tensor %d has %lld elements, outside 1..2^31-1", t, (long long)numel[t]);
        total += chunks_of(numel[t]);
    }
    if (total > kMaxNumel) return fail(-3, "plan: %lld chunks in all, above 2^31-1", (long long)total);
    *n_chunks = total;
    if (!chunks) return 0;
    if (capacity < total) return fail(-5, "plan: room for %lld chunk pairs, %lld needed", (long long)capacity, (long long)total);
    int64_t at = 0;
    for (int t = 0; t < n_tensors; ++t)
        for (int64_t k = 0, n = chunks_of(numel[t]); k < n; ++k, ++at) {
            chunks[2 * at] = t;
            chunks[2 * at + 1] = (int32_t)k;
        }
    return 0;
}

__attribute__((visibility("default"))) int ccnet_sgdmp_step(const int64_t *tensors_host, const int64_t *tensors_device,
                                                            int n_tensors, const int32_t *chunks_host,
                                                            const int32_t *chunks_device, int64_t n_chunks, const float *lr,
                                                            const float *wd, const float *mu, int n_groups,
                                                            const float *schedule, int schedule_len, int32_t *counter,
                                                            int zero_grads, int cap, void *stream) {
    if (!tensors_host || !tensors_device || !chunks_host || !chunks_device)
        return fail(-2, "step: NULL tensor table or chunk table (host or device copy)");
    if (!lr || !wd || !mu) return fail(-2, "step: NULL lr, wd or mu");
    if (n_tensors < 1 || n_tensors > CCNET_SGD_MAX_TENSORS)
        return fail(-1, "step: %d tensors, outside 1..%d", n_tensors, CCNET_SGD_MAX_TENSORS);
    if (n_groups < 1 || n_groups > CCNET_SGD_MAX_GROUPS)
        return fail(-6, "step: %d groups, outside 1..%d", n_groups, CCNET_SGD_MAX_GROUPS);
    if (cap < 0) return fail(-1, "step: cap %d is negative", cap);
    if (schedule && !counter) return fail(-7, "step: a schedule needs a counter");
    if (schedule && schedule_len < 1) return fail(-7, "step: schedule of length %d", schedule_len);
    int64_t at = 0;
    for (int t = 0; t < n_tensors; ++t) {
        const int64_t *row = tensors_host + (size_t)t * CCNET_SGDMP_TENSOR_WORDS;
        const int64_t numel = row[CCNET_SGDMP_NUMEL], group = row[CCNET_SGDMP_GROUP];
        if (numel < 1 || numel > kMaxNumel)
            return fail(-3, "step: tensor %d has %lld elements, outside 1..2^31-1", t, (long long)numel);
        if (group < 0 || group >= n_groups)
            return fail(-6, "step: tensor %d is in group %lld of %d", t, (long long)group, n_groups);
        if (!row[CCNET_SGDMP_P] || !row[CCNET_SGDMP_B]) return fail(-8, "step: tensor %d has a NULL parameter or momentum buffer", t);
        if (row[CCNET_SGDMP_M]) {
            if ((row[CCNET_SGDMP_M] | row[CCNET_SGDMP_B]) & 3)
                return fail(-8, "step: tensor %d has a master or momentum buffer that is not 4-byte aligned", t);
            if ((row[CCNET_SGDMP_P] | row[CCNET_SGDMP_G]) & 1)
                return fail(-8, "step: tensor %d has a bf16 parameter or gradient that is not 2-byte aligned", t);
        } else if ((row[CCNET_SGDMP_P] | row[CCNET_SGDMP_G] | row[CCNET_SGDMP_B]) & 3) {
            return fail(-8, "step: tensor %d has a parameter, gradient or momentum buffer that is not 4-byte aligned", t);
        }
        for (int64_t k = 0, n = chunks_of(numel); k < n; ++k, ++at) {
            if (at >= n_chunks || chunks_host[2 * at] != t || chunks_host[2 * at + 1] != k)
                return fail(-5, "step: chunk table differs from the plan at entry %lld (tensor %d, chunk %lld)", (long long)at, t,
                            (long long)k);
        }
    }
    if (at != n_chunks) return fail(-5, "step: chunk table has %lld entries, the plan %lld", (long long)n_chunks, (long long)at);
    if (at > kMaxNumel) return fail(-3, "step: %lld chunks in all, above 2^31-1", (long long)at);

    sgdmp::Hyper h;
    for (int q = 0; q < CCNET_SGD_MAX_GROUPS; ++q) {
        h.lr[q] = q < n_groups ? lr[q] : 0.f;
        h.wd[q] = q < n_groups ? wd[q] : 0.f;
        h.mu[q] = q < n_groups ? mu[q] : 0.f;
    }
    const int64_t limit = cap > 0 ? cap : CCNET_SGD_DEFAULT_CAP;
    const dim3 grid((unsigned)(n_chunks < limit ? n_chunks : limit));
    hipStream_t s = static_cast<hipStream_t>(stream);
    SGDMP_LAUNCH(sgdmp::step_kernel, grid, dim3(sgdmp::kThreads), s, tensors_device, chunks_device, (int)n_chunks, h, schedule,
                 schedule ? schedule_len : 0, schedule ? counter : nullptr, zero_grads);
    if (int code = launched("step")) return code;
    if (schedule) {
        SGDMP_LAUNCH(sgdmp::advance_kernel, dim3(1), dim3(1), s, counter);
        return launched("advance");
    }
    return 0;
}

}  // extern "C"
