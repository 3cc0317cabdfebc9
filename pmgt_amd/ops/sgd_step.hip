// Fused clip + SGD over a flat fp32 buffer (pmgt_op_sgd of include/pmgt_ops.h): torch.optim.SGD as the reference builds it under --optim sgd
// (pmgt/base_trainer.py:61-66: no momentum, COUPLED weight decay on the tensors get_optimizer lets decay), after clip_grad_norm_(max_norm)
// and under a LambdaLR stepped per optimizer step.  Three launches in the shape of every optimizer entry here, no sync, no allocation, no
// atomics:
//   1  sqnorm_part_kernel of csrc/optim.hip: the gradient norm has the AdamW entries' bits
//   2  the prepare lane of optimizer_step.hip (launch_step_prepare) with beta1 = beta2 = 0: its bias corrections are then 1 - 0^t = 1 exactly,
//      so it leaves scal[1] = (float)(lr_t / 1) = lr_t and scal[2] = (float)(1 / sqrt(1)) = 1, and the clip, lr_t = lr * lambda(*step), the
//      guard's decision, the counters and the log row are that lane's own code: the same bits as pmgt_op_adamw_guarded / pmgt_op_lr_schedule
//   3  sgd_update_kernel below
// The update is compiled WITHOUT contraction (as the LayerNorm statistics of ncf_model_train.hip are): every product and sum is rounded to
// fp32 in the order written, which is what lets a numpy fp32 restatement (pair_train.sgd_step_host) agree bit for bit.
#include <cmath>

#include "optimizer_step.h"

namespace pmgt {

__global__ void sqnorm_part_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ part);      // csrc/optim.hip

static __device__ __forceinline__ float sgd_element(float p, float g, bool decays, float clip, float lr_t, float wd) {
#pragma clang fp contract(off)
    const float gc = g * clip;
    const float d = decays ? gc + wd * p : gc;
    return p - lr_t * d;
}

// head: the floats in front of the first 16-byte boundary of p (0..3, at most n); the body is whole f32x4 from there, grid-stride; the tail
// is what is left (0..3).  vec: g shares p's alignment (the body moves 16 bytes a lane; else element by element); dec4: the body's decay bytes
// can be read 4 at a time.  The element-by-element body is a CORRECTNESS fallback (strided 4-byte accesses; nothing times it): the trainers'
// parameters and gradients are whole allocations, or views at the same offset of both, and take the 16-byte body.  Head and tail are block 0's, one lane an element.  Guarded sits behind the skipped flag: scal[5] is one value
// for the whole grid, so the branch is uniform and a skipped step moves no parameter byte.
template <bool Guarded>
__global__ __launch_bounds__(256) void sgd_update_kernel(float* __restrict__ p, const float* __restrict__ g, const uint8_t* __restrict__ decay,
                                                         int64_t n, int64_t head, int64_t nvec, bool vec, bool dec4, float wd,
                                                         const float* __restrict__ scal) {
    if constexpr (Guarded) {
        if (scal[5] != 0.f) return;
    }
    const float clip = scal[0], lr_t = scal[4];
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nvec; v += stride) {
        const int64_t i = head + v * 4;
        if (vec) {
            f32x4 pp = *(const f32x4*)(p + i);
            const f32x4 gg = *(const f32x4*)(g + i);
            uint32_t dm;
            if (dec4) dm = *(const uint32_t*)(decay + i);
            else dm = (uint32_t)decay[i] | ((uint32_t)decay[i + 1] << 8) | ((uint32_t)decay[i + 2] << 16) | ((uint32_t)decay[i + 3] << 24);
#pragma unroll
            for (int k = 0; k < 4; ++k) pp[k] = sgd_element(pp[k], gg[k], ((dm >> (8 * k)) & 0xFFu) != 0, clip, lr_t, wd);
            *(f32x4*)(p + i) = pp;
        } else {
            for (int k = 0; k < 4; ++k) p[i + k] = sgd_element(p[i + k], g[i + k], decay[i + k] != 0, clip, lr_t, wd);
        }
    }
    if (blockIdx.x == 0) {
        const int64_t t = threadIdx.x, tail = head + nvec * 4;
        if (t < head) p[t] = sgd_element(p[t], g[t], decay[t] != 0, clip, lr_t, wd);
        if (tail + t < n) p[tail + t] = sgd_element(p[tail + t], g[tail + t], decay[tail + t] != 0, clip, lr_t, wd);
    }
}

}  // namespace pmgt

using namespace pmgt;

extern "C" int pmgt_op_sgd(float* p, const float* g, const uint8_t* decay, int64_t n, float lr, float wd, float max_norm, int64_t* step,
                           float* scal, float* part, const pmgt_lr_schedule* sched, const pmgt_step_guard* guard, void* stream) {
    const char* who = "pmgt_op_sgd";
    PMGT_CHECK(p && g && decay && step && scal && part, -2, "%s: NULL argument", who);
    PMGT_CHECK(n >= 0, -2, "%s: n = %lld is negative", who, (long long)n);
    PMGT_CHECK(std::isfinite(lr) && std::isfinite(wd) && std::isfinite(max_norm), -2, "%s: lr = %g, wd = %g or max_norm = %g is not finite", who,
               (double)lr, (double)wd, (double)max_norm);
    LrSchedule s;
    if (int rc = schedule_from(sched, true, lr, who, &s)) return rc;
    StepGuard gd;
    if (guard != nullptr)
        if (int rc = guard_from(guard, who, &gd)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    const int nparts = (int)std::min<int64_t>(1024, cdiv64(n, 1024));
    if (nparts > 0) {
        hipLaunchKernelGGL(sqnorm_part_kernel, dim3(nparts), dim3(256), 0, st, g, n, part);
        PMGT_LAUNCH_OK();
    }
    if (int rc = launch_step_prepare(part, nparts, max_norm, lr, 0.f, 0.f, step, scal, s, guard ? &gd : nullptr, st)) return rc;
    if (n == 0) return 0;
    const int64_t head = std::min<int64_t>(n, (int64_t)(((16 - ((uintptr_t)p & 15)) & 15) / 4)), nvec = (n - head) / 4;
    const bool vec = ((uintptr_t)(p + head) & 15) == 0 && ((uintptr_t)(g + head) & 15) == 0, dec4 = ((uintptr_t)(decay + head) & 3) == 0;
    // 8 blocks a CU on 256 CUs keep HBM busy; beyond that the grid strides
    const unsigned blocks = (unsigned)std::min<int64_t>(2048, std::max<int64_t>(1, cdiv64(nvec, 256)));
    const auto update = guard ? sgd_update_kernel<true> : sgd_update_kernel<false>;
    hipLaunchKernelGGL(update, dim3(blocks), dim3(256), 0, st, p, g, decay, n, head, nvec, vec, dec4, wd, scal);
    PMGT_LAUNCH_OK();
    return 0;
}
