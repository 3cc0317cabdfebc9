// The guarded form of the fused clip + AdamW step (csrc/optim.hip, ops/lr_schedule.hip) and its entry points
// (pmgt_optimizer_step_guarded of include/pmgt_capi.h; pmgt_op_adamw_guarded of include/pmgt_ops.h).
// What a GradScaler gives the reference under --mp-enabled (pmgt/base_trainer.py:312): an optimizer step whose gradients hold an Inf or
// a NaN is SKIPPED.  The decision is taken in the single-lane prepare kernel, from the global gradient norm it computes anyway, so a
// captured step carries it with no host `if` between backward and optimizer; the same lane keeps the attempt / skip counters and one
// row per step of a log ring (loss, pre-clip norm, clip coefficient, rate), which is what a replayed run can be watched by without a
// host sync per step.
// "Bad" = the norm is not finite.  That is any Inf or NaN gradient element, and also finite gradients whose sum of squares overflows
// the fp32 partials of sqnorm_part_kernel: torch.nn.utils.clip_grad_norm_ on fp32 gradients reports the same Inf norm for those.
// Kept out of csrc/ for lr_schedule.hip's reason: the unguarded step and every kernel bench.py measures stay byte for byte what they
// were.  The step is the same three launches (csrc/optim.hip's norm partials, prepare, AdamW), no sync, no allocation.
//
// Log ring (pmgt_step_guard): row r = attempt index % log_rows.
//   log_f [log_rows][PMGT_STEP_LOG_FLOATS = 8] fp32: [0] loss (NaN with a NULL loss pointer), [1] pre-clip gradient norm, [2] clip
//     coefficient (0 on a skipped step), [3] lr_t, [4] flag: 0 = applied, 1 = skipped, 2 = applied although the norm is not finite
//     (skip_nonfinite = 0); [5..7] are not written
//   log_i [log_rows][2] int64: [0] attempt index (0-based, counted over applied and skipped steps), [1] opt_step after the step
#include "lr_schedule.h"

namespace pmgt {

__global__ void sqnorm_part_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ part);      // csrc/optim.hip

struct StepGuard {
    int64_t* counters;      // [4]: attempts, skipped, skipped in a row, reserved
    float* log_f;           // [log_rows][8] or NULL
    int64_t* log_i;         // [log_rows][2] or NULL
    int64_t log_rows;
    const float* loss;      // device scalar or NULL
    int skip_nonfinite;
};

// adam_prepare_scheduled_kernel of lr_schedule.hip -- the same arithmetic in the same order on a step that is applied -- with the
// decision, the counters and the log.  scal [8]: [0] = clip coefficient, [1] = lr_t / bc1, [2] = 1 / sqrt(bc2), [3] = total grad norm
// (pre-clip), [4] = lr_t, [5] = 1 when the step is skipped, else 0; [6..7] are not written.  A skipped step leaves step[0], scal[1]
// and scal[2] alone: the bias corrections and the schedule count applied steps only.
__global__ __launch_bounds__(64) void adam_prepare_guarded_kernel(const float* __restrict__ part, int nparts, float max_norm, float lr, float b1,
                                                                  float b2, int64_t* __restrict__ step, float* __restrict__ scal,
                                                                  const LrSchedule sched, const StepGuard gd) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 64) s += (double)part[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) {
        const double norm = sqrt(s);
        const bool bad = !isfinite(norm), skip = bad && gd.skip_nonfinite != 0;
        int64_t t = step[0];
        double coef = 0.0, lr_t;
        if (skip) {
            lr_t = scheduled_lr(sched, (double)lr, t);      // the rate the step would have used
            scal[0] = 0.f;
        } else {
            t += 1;
            step[0] = t;
            coef = 1.0;
            if (max_norm > 0.f) coef = fmin((double)max_norm / (norm + 1e-6), 1.0);
            const double bc1 = 1.0 - pow((double)b1, (double)t), bc2 = 1.0 - pow((double)b2, (double)t);
            lr_t = scheduled_lr(sched, (double)lr, t - 1);
            scal[0] = (float)coef;
            scal[1] = (float)(lr_t / bc1);
            scal[2] = (float)(1.0 / sqrt(bc2));
        }
        scal[3] = (float)norm;
        scal[4] = (float)lr_t;
        scal[5] = skip ? 1.f : 0.f;
        const int64_t attempt = gd.counters[0];
        gd.counters[0] = attempt + 1;
        if (skip) {
            gd.counters[1] += 1;
            gd.counters[2] += 1;
        } else {
            gd.counters[2] = 0;
        }
        if (gd.log_rows > 0) {
            const int64_t r = attempt % gd.log_rows;
            float* f = gd.log_f + r * PMGT_STEP_LOG_FLOATS;
            f[0] = gd.loss ? gd.loss[0] : __builtin_nanf("");
            f[1] = (float)norm;
            f[2] = (float)coef;
            f[3] = (float)lr_t;
            f[4] = skip ? 1.f : (bad ? 2.f : 0.f);
            gd.log_i[r * 2 + 0] = attempt;
            gd.log_i[r * 2 + 1] = t;
        }
    }
}

// adamw_scheduled_kernel of lr_schedule.hip, the same arithmetic in the same order, behind the skipped flag: scal[5] is one value for
// the whole grid, so the branch is uniform and a skipped step moves no parameter byte
__global__ __launch_bounds__(256) void adamw_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, const uint8_t* __restrict__ decay, int64_t n, float wd,
                                                            float b1, float b2, float eps, const float* __restrict__ scal) {
    if (scal[5] != 0.f) return;
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

static int guard_from(const pmgt_step_guard* in, const char* who, StepGuard* out) {
    PMGT_CHECK(in != nullptr, -2, "%s: NULL guard", who);
    PMGT_CHECK(in->counters != nullptr, -2, "%s: NULL guard counters", who);
    PMGT_CHECK(in->log_rows >= 0, -2, "%s: log_rows = %lld is negative", who, (long long)in->log_rows);
    PMGT_CHECK(in->log_rows == 0 || (in->log_f && in->log_i), -2, "%s: log_rows = %lld but a log pointer is NULL", who, (long long)in->log_rows);
    *out = StepGuard{in->counters, in->log_f, in->log_i, in->log_rows, in->loss, in->skip_nonfinite};
    return 0;
}

// adamw_step of csrc/optim.hip: norm partials -> prepare -> AdamW, three launches
static int adamw_step_guarded(const AdamArgs& a, const LrSchedule& sched, const StepGuard& gd, hipStream_t st) {
    if (a.n <= 0) return 0;
    const int nparts = (int)std::min<int64_t>(1024, cdiv64(a.n, 1024));
    hipLaunchKernelGGL(sqnorm_part_kernel, dim3(nparts), dim3(256), 0, st, a.g, a.n, a.part);
    PMGT_LAUNCH_OK();
    hipLaunchKernelGGL(adam_prepare_guarded_kernel, dim3(1), dim3(64), 0, st, a.part, nparts, a.max_norm, a.lr, a.b1, a.b2, a.step, a.scal, sched,
                       gd);
    PMGT_LAUNCH_OK();
    hipLaunchKernelGGL(adamw_guarded_kernel, dim3((unsigned)cdiv64(cdiv64(a.n, 4), 256)), dim3(256), 0, st, a.p, a.g, a.m, a.v, a.decay, a.n,
                       a.wd, a.b1, a.b2, a.eps, a.scal);
    PMGT_LAUNCH_OK();
    return 0;
}

// a NULL schedule is the constant rate: lambda = 1, so lr_t = (double)lr and the step is pmgt_optimizer_step's bit for bit
static int schedule_or_constant(const pmgt_lr_schedule* in, float lr, const char* who, LrSchedule* out) {
    if (in == nullptr) {
        *out = LrSchedule{PMGT_LR_CONSTANT, 0, 0};
        return 0;
    }
    return schedule_from(in, lr, who, out);
}

}  // namespace pmgt

using namespace pmgt;

extern "C" {

int pmgt_optimizer_step_guarded(pmgt_engine* e, const pmgt_tensors* t, const pmgt_adam* a, const pmgt_lr_schedule* sched,
                                const pmgt_step_guard* guard, void* stream) {
    PMGT_CHECK(e && t && a && t->params && t->grads && a->exp_avg && a->exp_avg_sq && a->decay && a->step && a->scalars && a->scratch,
               -2, "pmgt_optimizer_step_guarded: NULL argument");
    LrSchedule s;
    if (int rc = schedule_or_constant(sched, a->lr, "pmgt_optimizer_step_guarded", &s)) return rc;
    StepGuard gd;
    if (int rc = guard_from(guard, "pmgt_optimizer_step_guarded", &gd)) return rc;
    AdamArgs x;
    x.p = t->params; x.g = t->grads; x.m = a->exp_avg; x.v = a->exp_avg_sq; x.decay = a->decay; x.n = pmgt_param_count(e);
    x.lr = a->lr; x.wd = a->weight_decay; x.b1 = a->beta1; x.b2 = a->beta2; x.eps = a->eps; x.max_norm = a->max_grad_norm;
    x.step = a->step; x.scal = a->scalars; x.part = a->scratch;
    return adamw_step_guarded(x, s, gd, (hipStream_t)stream);
}

int pmgt_op_adamw_guarded(float* p, const float* g, float* m, float* v, const uint8_t* decay, int64_t n, float lr, float wd, float b1,
                          float b2, float eps, float max_norm, int64_t* step, float* scal, float* part, const pmgt_lr_schedule* sched,
                          const pmgt_step_guard* guard, void* stream) {
    LrSchedule s;
    if (int rc = schedule_or_constant(sched, lr, "pmgt_op_adamw_guarded", &s)) return rc;
    StepGuard gd;
    if (int rc = guard_from(guard, "pmgt_op_adamw_guarded", &gd)) return rc;
    AdamArgs a;
    a.p = p; a.g = g; a.m = m; a.v = v; a.decay = decay; a.n = n; a.lr = lr; a.wd = wd; a.b1 = b1; a.b2 = b2; a.eps = eps;
    a.max_norm = max_norm; a.step = step; a.scal = scal; a.part = part;
    return adamw_step_guarded(a, s, gd, (hipStream_t)stream);
}

}  // extern "C"
