// Learning-rate schedule evaluated on the device: the scheduled form of the fused clip + AdamW step (csrc/optim.hip) and its entry points
// (pmgt_optimizer_step_scheduled of include/pmgt_capi.h; pmgt_op_adamw_scheduled / pmgt_op_lr_schedule of include/pmgt_ops.h).
// The prepare kernel computes lr_t = lr * lambda(steps completed so far) from the device-side step counter, so a captured step follows the
// schedule with no re-capture and no host write between replays.  lambda: the multipliers of transformers 4.11.2 optimization.py with the
// defaults get_scheduler leaves in place (the reference: --scheduler-type / --scheduler-warmup, train.py:38-52, pmgt/base_trainer.py:71-90).
// Kept out of csrc/: the unscheduled step and every kernel bench.py measures (and fingerprints there) stay byte for byte what they were; the
// gradient-norm partials are csrc/optim.hip's own kernel, so the step is the same three launches.
#include "lr_schedule.h"      // LrSchedule, scheduled_lr, schedule_from: shared with guarded_step.hip

namespace pmgt {

__global__ void sqnorm_part_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ part);      // csrc/optim.hip

// adam_prepare_kernel of csrc/optim.hip with lr_t for lr.  scal [8]: [0] = clip coefficient, [1] = lr_t / bc1, [2] = 1 / sqrt(bc2),
// [3] = total grad norm (pre-clip), [4] = lr_t; [5..7] are not written
__global__ __launch_bounds__(64) void adam_prepare_scheduled_kernel(const float* __restrict__ part, int nparts, float max_norm, float lr, float b1,
                                                                    float b2, int64_t* __restrict__ step, float* __restrict__ scal,
                                                                    const LrSchedule sched) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 64) s += (double)part[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) {
        const int64_t t = step[0] + 1;
        step[0] = t;
        const double norm = sqrt(s);
        double coef = 1.0;
        if (max_norm > 0.f) coef = fmin((double)max_norm / (norm + 1e-6), 1.0);
        const double bc1 = 1.0 - pow((double)b1, (double)t), bc2 = 1.0 - pow((double)b2, (double)t);
        const double lr_t = scheduled_lr(sched, (double)lr, t - 1);
        scal[0] = (float)coef;
        scal[1] = (float)(lr_t / bc1);
        scal[2] = (float)(1.0 / sqrt(bc2));
        scal[3] = (float)norm;
        scal[4] = (float)lr_t;
    }
}

// adamw_kernel of csrc/optim.hip, the same arithmetic in the same order, with the decay term's rate read from scal[4]
__global__ __launch_bounds__(256) void adamw_scheduled_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                              float* __restrict__ v, const uint8_t* __restrict__ decay, int64_t n, float wd,
                                                              float b1, float b2, float eps, const float* __restrict__ scal) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const float coef = scal[0], step_size = scal[1], inv_sqrt_bc2 = scal[2], lr = scal[4];
    const int cnt = (int)min((int64_t)4, n - i);
    for (int k = 0; k < cnt; ++k) {
        const int64_t j = i + k;
        const float gg = g[j] * coef;
        float pp = p[j] * (1.f - lr * (decay[j] ? wd : 0.f));
        const float mm = m[j] * b1 + gg * (1.f - b1);
        const float vv = v[j] * b2 + gg * gg * (1.f - b2);
        const float denom = sqrtf(vv) * inv_sqrt_bc2 + eps;
        pp -= step_size * (mm / denom);
        p[j] = pp; m[j] = mm; v[j] = vv;
    }
}

__global__ __launch_bounds__(256) void lr_schedule_kernel(const LrSchedule sched, float lr, int64_t first_step, int n, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (float)scheduled_lr(sched, (double)lr, first_step + i);
}

// adamw_step of csrc/optim.hip: norm partials -> prepare -> AdamW, three launches
static int adamw_step_scheduled(const AdamArgs& a, const LrSchedule& sched, hipStream_t st) {
    if (a.n <= 0) return 0;
    const int nparts = (int)std::min<int64_t>(1024, cdiv64(a.n, 1024));
    hipLaunchKernelGGL(sqnorm_part_kernel, dim3(nparts), dim3(256), 0, st, a.g, a.n, a.part);
    PMGT_LAUNCH_OK();
    hipLaunchKernelGGL(adam_prepare_scheduled_kernel, dim3(1), dim3(64), 0, st, a.part, nparts, a.max_norm, a.lr, a.b1, a.b2, a.step, a.scal, sched);
    PMGT_LAUNCH_OK();
    hipLaunchKernelGGL(adamw_scheduled_kernel, dim3((unsigned)cdiv64(cdiv64(a.n, 4), 256)), dim3(256), 0, st, a.p, a.g, a.m, a.v, a.decay, a.n,
                       a.wd, a.b1, a.b2, a.eps, a.scal);
    PMGT_LAUNCH_OK();
    return 0;
}

}  // namespace pmgt

using namespace pmgt;

extern "C" {

int pmgt_optimizer_step_scheduled(pmgt_engine* e, const pmgt_tensors* t, const pmgt_adam* a, const pmgt_lr_schedule* sched, void* stream) {
    PMGT_CHECK(e && t && a && sched && t->params && t->grads && a->exp_avg && a->exp_avg_sq && a->decay && a->step && a->scalars && a->scratch,
               -2, "pmgt_optimizer_step_scheduled: NULL argument");
    LrSchedule s;
    if (int rc = schedule_from(sched, a->lr, "pmgt_optimizer_step_scheduled", &s)) return rc;
    AdamArgs x;
    x.p = t->params; x.g = t->grads; x.m = a->exp_avg; x.v = a->exp_avg_sq; x.decay = a->decay; x.n = pmgt_param_count(e);
    x.lr = a->lr; x.wd = a->weight_decay; x.b1 = a->beta1; x.b2 = a->beta2; x.eps = a->eps; x.max_norm = a->max_grad_norm;
    x.step = a->step; x.scal = a->scalars; x.part = a->scratch;
    return adamw_step_scheduled(x, s, (hipStream_t)stream);
}

int pmgt_op_adamw_scheduled(float* p, const float* g, float* m, float* v, const uint8_t* decay, int64_t n, float lr, float wd, float b1,
                            float b2, float eps, float max_norm, int64_t* step, float* scal, float* part, const pmgt_lr_schedule* sched,
                            void* stream) {
    LrSchedule s;
    if (int rc = schedule_from(sched, lr, "pmgt_op_adamw_scheduled", &s)) return rc;
    AdamArgs a;
    a.p = p; a.g = g; a.m = m; a.v = v; a.decay = decay; a.n = n; a.lr = lr; a.wd = wd; a.b1 = b1; a.b2 = b2; a.eps = eps;
    a.max_norm = max_norm; a.step = step; a.scal = scal; a.part = part;
    return adamw_step_scheduled(a, s, (hipStream_t)stream);
}

int pmgt_op_lr_schedule(const pmgt_lr_schedule* sched, float lr, int64_t first_step, int n, float* out, void* stream) {
    LrSchedule s;
    if (int rc = schedule_from(sched, lr, "pmgt_op_lr_schedule", &s)) return rc;
    PMGT_CHECK(out || n <= 0, -2, "pmgt_op_lr_schedule: NULL output");
    if (n <= 0) return 0;
    hipLaunchKernelGGL(lr_schedule_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, (hipStream_t)stream, s, lr, first_step, n, out);
    PMGT_LAUNCH_OK();
    return 0;
}

}  // extern "C"
