// Fused clip + SGD over a flat fp32 buffer (pmgt_op_sgd of include/pmgt_ops.h): torch.optim.SGD as the reference builds it under --optim sgd
// (pmgt/base_trainer.py:61-66: no momentum, COUPLED weight decay on the tensors get_optimizer lets decay), after clip_grad_norm_(max_norm)
// and under a LambdaLR stepped per optimizer step.  Three launches in the shape of every optimizer entry here, no sync, no allocation, no
// atomics:
//   1  sqnorm_part_kernel of csrc/optim.hip: the gradient norm has the AdamW entries' bits
//   2  the prepare lane of optimizer_step.hip (launch_step_prepare) with beta1 = beta2 = 0: its bias corrections are then 1 - 0^t = 1 exactly,
//      so it leaves scal[1] = (float)(lr_t / 1) = lr_t and scal[2] = (float)(1 / sqrt(1)) = 1, and the clip, lr_t = lr * lambda(*step), the
//      guard's decision, the counters and the log row are that lane's own code: the same bits as pmgt_op_adamw_guarded / pmgt_op_lr_schedule
//   3  sgd_update_kernel below
// The update (sgd_element of optimizer_step.h, which pmgt_op_step_segments shares) is compiled WITHOUT contraction (as the LayerNorm statistics
// of ncf_model_train.hip are): every product and sum is rounded to fp32 in the order written, which is what lets a numpy fp32 restatement
// (pair_train.sgd_step_host) agree bit for bit.
#include <cmath>

#include "optimizer_step.h"

namespace pmgt {

__global__ void sqnorm_part_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ part);      // csrc/optim.hip

// sgd_update_range of optimizer_step.h (the head / 16-byte body / tail walk over sgd_element) at the rate scal[4].  Guarded sits behind the
// skipped flag: scal[5] is one value for the whole grid, so the branch is uniform and a skipped step moves no parameter byte.
template <bool Guarded>
__global__ __launch_bounds__(256) void sgd_update_kernel(float* __restrict__ p, const float* __restrict__ g, const uint8_t* __restrict__ decay,
                                                         int64_t n, int64_t head, int64_t nvec, bool vec, bool dec4, float wd,
                                                         const float* __restrict__ scal) {
    if constexpr (Guarded) {
        if (scal[5] != 0.f) return;
    }
    sgd_update_range(p, g, decay, n, head, nvec, vec, dec4, wd, scal[0], scal[4]);
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
    const SgdSplit sp = sgd_split(p, g, decay, n);
    const auto update = guard ? sgd_update_kernel<true> : sgd_update_kernel<false>;
    hipLaunchKernelGGL(update, dim3(sp.blocks), dim3(256), 0, st, p, g, decay, n, sp.head, sp.nvec, sp.vec, sp.dec4, wd, scal);
    PMGT_LAUNCH_OK();
    return 0;
}
