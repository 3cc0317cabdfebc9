// Weight averaging over the flat fp32 parameter buffer (pmgt_weight_average_update / pmgt_weight_swap of include/pmgt_capi.h, which states
// the device state layout): the arithmetic of the reference's swa_step and the content exchange of its swap_swa_params
// (pmgt/utils/train.py:53-85, driven by the StochasticWeightAveraging callback, pmgt/callbacks.py:44-381), plus a per-step exponential
// average that lives inside a captured step.
//   avg_apply    avg[j] = avg[j] * w_old + p[j] * w_new: two products and one sum, each rounded to fp32 on its own (no fused
//                multiply-add), so a numpy fp32 restatement matches bit for bit.  The weights come by value (SWA: the host knows the
//                model count) or from the device state an EARLIER launch wrote (EMA); the device form sits behind the state's skip word,
//                one value for the whole grid, so the branch is uniform and a skipped step moves no byte -- adamw_step_kernel<true>'s rule.
//   avg_prepare  one lane, as adam_prepare_step_kernel: reads the optimizer's skipped flag (scal[5]; NULL = never skipped), and either sets
//                the skip word and leaves the count alone, or writes both weights from the fp64 decay of this update, clears the skip word
//                and counts the update.
//   swap         exchanges two buffers as raw 32-bit words: NaN payloads and signed zeros move unchanged.
// All of them stream from HBM with no reuse: 16-byte accesses (four fp32 per lane) over the body, a scalar tail of < 4 elements, one
// group per lane at 256 lanes per block (12 bytes of traffic per element leave nothing to hide behind more work per lane).  Base pointers
// that are not 16-byte aligned take the scalar form of the same kernel.  No LDS, no atomics, no allocation, no sync, no environment reads.
// Kept out of csrc/ for optimizer_step.hip's reason: the measured step launches nothing of this.
#include "../../include/pmgt_capi.h"
#include "../csrc/common.h"

namespace pmgt {

// the device state, PMGT_AVG_STATE_BYTES: int64 [0] n_upd; then 32-bit words [2] skip word, [3] w_old (fp32), [4] w_new (fp32), [5..7] reserved
struct AvgState {
    int64_t n_upd;
    uint32_t skip;
    float w_old, w_new;
    uint32_t reserved[3];
};
static_assert(sizeof(AvgState) == PMGT_AVG_STATE_BYTES, "pmgt_capi.h states this layout");

__global__ __launch_bounds__(64) void avg_prepare_kernel(AvgState* __restrict__ st, const float* __restrict__ skip_flag, double decay, int warmup) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (skip_flag != nullptr && skip_flag[0] != 0.f) {
        st->skip = 1u;
        return;
    }
    const int64_t n = st->n_upd;
    double d = decay;
    if (warmup) d = fmin(decay, (1.0 + (double)n) / (10.0 + (double)n));
    st->w_old = (float)d;
    st->w_new = (float)(1.0 - d);
    st->skip = 0u;
    st->n_upd = n + 1;
}

// three roundings.  __fmul_rn / __fadd_rn alone do not bind hipcc (it fuses the second product into a v_fmac_f32 under its default
// -ffp-contract=fast-honor-pragmas): the pragma does, as in eval_metrics.hip, and it survives the inlining (no `contract` flag in the IR)
__device__ __forceinline__ float avg_one(float a, float p, float w_old, float w_new) {
#pragma clang fp contract(off)
    const float x = a * w_old;
    const float y = p * w_new;
    return x + y;
}

// FromState: weights and skip word from `st`; else by value.  Vec: 16-byte body (both bases 16-byte aligned).
template <bool FromState, bool Vec>
__global__ __launch_bounds__(256) void avg_apply_kernel(float* __restrict__ avg, const float* __restrict__ p, int64_t n, float w_old, float w_new,
                                                        const AvgState* __restrict__ st) {
    if constexpr (FromState) {
        if (st->skip != 0u) return;
        w_old = st->w_old;
        w_new = st->w_new;
    }
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    if (Vec && i + 4 <= n) {
        float4 a = *reinterpret_cast<const float4*>(avg + i);
        const float4 q = *reinterpret_cast<const float4*>(p + i);
        a.x = avg_one(a.x, q.x, w_old, w_new);
        a.y = avg_one(a.y, q.y, w_old, w_new);
        a.z = avg_one(a.z, q.z, w_old, w_new);
        a.w = avg_one(a.w, q.w, w_old, w_new);
        *reinterpret_cast<float4*>(avg + i) = a;
        return;
    }
    const int cnt = (int)min((int64_t)4, n - i);
    for (int k = 0; k < cnt; ++k) avg[i + k] = avg_one(avg[i + k], p[i + k], w_old, w_new);
}

template <bool Vec>
__global__ __launch_bounds__(256) void swap_kernel(uint32_t* __restrict__ a, uint32_t* __restrict__ b, int64_t n) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    if (Vec && i + 4 <= n) {
        const uint4 x = *reinterpret_cast<const uint4*>(a + i);
        const uint4 y = *reinterpret_cast<const uint4*>(b + i);
        *reinterpret_cast<uint4*>(a + i) = y;
        *reinterpret_cast<uint4*>(b + i) = x;
        return;
    }
    const int cnt = (int)min((int64_t)4, n - i);
    for (int k = 0; k < cnt; ++k) {
        const uint32_t x = a[i + k], y = b[i + k];
        a[i + k] = y;
        b[i + k] = x;
    }
}

static inline bool aligned16(const void* a, const void* b) {
    return (((uintptr_t)a | (uintptr_t)b) & 15u) == 0;
}
static inline dim3 groups_grid(int64_t n) {
    return dim3((unsigned)cdiv64(cdiv64(n, 4), 256));
}

}  // namespace pmgt

using namespace pmgt;

extern "C" {

int pmgt_weight_average_update(float* avg, const float* params, int64_t n, const pmgt_avg_step* cfg, void* stream) {
    PMGT_CHECK(avg != nullptr && params != nullptr, -2, "pmgt_weight_average_update: NULL buffer");
    PMGT_CHECK(cfg != nullptr, -2, "pmgt_weight_average_update: NULL cfg");
    PMGT_CHECK(n >= 0, -2, "pmgt_weight_average_update: n = %lld is negative", (long long)n);
    PMGT_CHECK(n < ((int64_t)1 << 41), -2, "pmgt_weight_average_update: n = %lld is past the launch grid", (long long)n);
    PMGT_CHECK(cfg->mode == PMGT_AVG_SWA || cfg->mode == PMGT_AVG_EMA, -2, "pmgt_weight_average_update: unknown mode %d", cfg->mode);
    hipStream_t st = (hipStream_t)stream;
    const bool vec = aligned16(avg, params);
    if (cfg->mode == PMGT_AVG_SWA) {
        if (n == 0) return 0;
        const auto apply = vec ? avg_apply_kernel<false, true> : avg_apply_kernel<false, false>;
        hipLaunchKernelGGL(apply, groups_grid(n), dim3(256), 0, st, avg, params, n, cfg->w_old, cfg->w_new, (const AvgState*)nullptr);
        PMGT_LAUNCH_OK();
        return 0;
    }
    PMGT_CHECK(cfg->decay >= 0.0 && cfg->decay < 1.0, -2, "pmgt_weight_average_update: decay = %g is outside [0, 1)", cfg->decay);
    PMGT_CHECK(cfg->state != nullptr, -2, "pmgt_weight_average_update: NULL device state");
    PMGT_CHECK(((uintptr_t)cfg->state & 7u) == 0, -2, "pmgt_weight_average_update: the device state is not 8-byte aligned");
    AvgState* state = (AvgState*)cfg->state;
    hipLaunchKernelGGL(avg_prepare_kernel, dim3(1), dim3(64), 0, st, state, cfg->skip_flag, cfg->decay, cfg->warmup != 0 ? 1 : 0);
    PMGT_LAUNCH_OK();
    if (n == 0) return 0;
    const auto apply = vec ? avg_apply_kernel<true, true> : avg_apply_kernel<true, false>;
    hipLaunchKernelGGL(apply, groups_grid(n), dim3(256), 0, st, avg, params, n, 0.f, 0.f, (const AvgState*)state);
    PMGT_LAUNCH_OK();
    return 0;
}

int pmgt_weight_swap(float* a, float* b, int64_t n, void* stream) {
    PMGT_CHECK(a != nullptr && b != nullptr, -2, "pmgt_weight_swap: NULL buffer");
    PMGT_CHECK(n >= 0, -2, "pmgt_weight_swap: n = %lld is negative", (long long)n);
    PMGT_CHECK(n < ((int64_t)1 << 41), -2, "pmgt_weight_swap: n = %lld is past the launch grid", (long long)n);
    PMGT_CHECK(a != b, -2, "pmgt_weight_swap: both buffers are the same");
    if (n == 0) return 0;
    const auto swap = aligned16(a, b) ? swap_kernel<true> : swap_kernel<false>;
    hipLaunchKernelGGL(swap, groups_grid(n), dim3(256), 0, (hipStream_t)stream, (uint32_t*)a, (uint32_t*)b, n);
    PMGT_LAUNCH_OK();
    return 0;
}

}  // extern "C"
