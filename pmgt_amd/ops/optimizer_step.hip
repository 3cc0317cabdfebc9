// The derived forms of the fused clip + AdamW step (csrc/optim.hip) -- scheduled, and scheduled + guarded -- as ONE kernel pair, and every
// optimizer entry point outside csrc/: pmgt_optimizer_step_scheduled / pmgt_optimizer_step_guarded of include/pmgt_capi.h (which states the
// scal [8] layout and the log ring), pmgt_op_adamw / pmgt_op_adamw_scheduled / pmgt_op_adamw_guarded / pmgt_op_lr_schedule of
// include/pmgt_ops.h.
// Scheduled: the prepare lane computes lr_t = lr * lambda(steps completed so far) from the device-side step counter, so a captured step
// follows the schedule with no re-capture and no host write between replays.  lambda: the multipliers of transformers 4.11.2
// optimization.py with the defaults get_scheduler leaves in place (the reference: --scheduler-type / --scheduler-warmup, train.py:38-52,
// pmgt/base_trainer.py:71-90).
// Guarded: what a GradScaler gives the reference under --mp-enabled (pmgt/base_trainer.py:312): a step whose gradients hold an Inf or a
// NaN is SKIPPED.  The same lane decides it, from the global gradient norm it computes anyway, so a captured step carries the decision
// with no host `if` between backward and optimizer; it also keeps the attempt / skip counters and one row per step of a log ring, which
// is what a replayed run can be watched by without a host sync per step.  "Bad" = the norm is not finite: any Inf or NaN gradient
// element, and also finite gradients whose sum of squares overflows the fp32 partials of sqnorm_part_kernel
// (torch.nn.utils.clip_grad_norm_ on fp32 gradients reports the same Inf norm for those).
// Kept out of csrc/: the plain step and every kernel bench.py measures (and fingerprints there) stay byte for byte what they were.  The
// gradient-norm partials are csrc/optim.hip's own kernel, so every form is the same three launches, no sync, no allocation.
// The checked schedule and guard and the launch of the prepare lane are declared in optimizer_step.h: sgd_step.hip (pmgt_op_sgd) prepares its
// step with this file's lane, so its clip, rate and guard are these kernels' bits.  The schedule (scheduled_lr) and the lane's body
// (prepare_step_lane) are device code of that header: segments_step.hip (pmgt_op_step_segments) runs the same lane over several segments.
// Segments (pmgt_op_adamw_segments): up to PMGT_ADAM_MAX_SEGMENTS disjoint flat buffers clipped by ONE global norm and stepped by one counter,
// each at a rate of its own -- an encoder fine-tuned through a head, two buffers, the encoder's learning rate its own.  One norm launch and
// one update launch per segment around one prepare launch.
#include <cmath>

#include "../../include/pmgt_ops.h"
#include "../csrc/optim.h"
#include "optimizer_step.h"

namespace pmgt {

__global__ void sqnorm_part_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ part);      // csrc/optim.hip

// The prepare lane: one wave adds the norm partials in fp64; its first thread runs prepare_step_lane of optimizer_step.h (the clip, lr_t, the
// bias corrections, the guard's decision, the counters and the log row).
template <bool Guarded>
__global__ __launch_bounds__(64) void adam_prepare_step_kernel(const float* __restrict__ part, int nparts, float max_norm, float lr, float b1,
                                                               float b2, int64_t* __restrict__ step, float* __restrict__ scal,
                                                               const LrSchedule sched, const StepGuard gd) {
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += 64) s += (double)part[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x != 0) return;
    prepare_step_lane<Guarded>(s, max_norm, lr, b1, b2, step, scal, sched, gd);
}

// adamw_kernel of csrc/optim.hip, the same fp32 arithmetic in the same order, with the decay term's rate read from scal[4].  Guarded sits
// behind the skipped flag: scal[5] is one value for the whole grid, so the branch is uniform and a skipped step moves no parameter byte.
template <bool Guarded>
__global__ __launch_bounds__(256) void adamw_step_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                         float* __restrict__ v, const uint8_t* __restrict__ decay, int64_t n, float wd,
                                                         float b1, float b2, float eps, const float* __restrict__ scal) {
    if constexpr (Guarded) {
        if (scal[5] != 0.f) return;
    }
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

// ---- several flat buffers as ONE optimizer (pmgt_op_adamw_segments): the norm over all of them, one clip coefficient, one step counter, one
// pair of bias corrections; per segment a rate of its own.  The partials of segment s are sqnorm_part_kernel's, at part + 1024 s.
// adam_prepare_kernel of csrc/optim.hip over the partials of every segment: a lane adds its partials of segment 0, then of segment 1, ..., in
// fp64 (ONE segment: that kernel's sum in that kernel's order, so the same bits); scal[4] = lr as the scheduled form leaves it
__global__ __launch_bounds__(64) void adam_prepare_segments_kernel(const float* __restrict__ part, const SegParts sp, float max_norm, float lr,
                                                                   float b1, float b2, int64_t* __restrict__ step, float* __restrict__ scal) {
    double s = 0.0;
    for (int k = 0; k < sp.count; ++k)
        for (int i = threadIdx.x; i < sp.nparts[k]; i += 64) s += (double)part[k * 1024 + i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x == 0) {
        const int64_t t = step[0] + 1;
        step[0] = t;
        const double norm = sqrt(s);
        double coef = 1.0;
        if (max_norm > 0.f) coef = fmin((double)max_norm / (norm + 1e-6), 1.0);
        const double bc1 = 1.0 - pow((double)b1, (double)t), bc2 = 1.0 - pow((double)b2, (double)t);
        scal[0] = (float)coef;
        scal[1] = (float)((double)lr / bc1);
        scal[2] = (float)(1.0 / sqrt(bc2));
        scal[3] = (float)norm;
        scal[4] = lr;
    }
}

// adamw_kernel of csrc/optim.hip, the same fp32 arithmetic in the same order, on one segment: the step size is scal[1] * lr_scale and the
// decay term's rate lr_seg = lr * lr_scale (the host's fp32 product); lr_scale == 1 multiplies by exactly 1: that kernel's bits.
// lr_scale == 0: p * (1 - 0) - 0 * (m / denom) = p bit for bit (denom >= eps > 0), while m and v move.
__global__ __launch_bounds__(256) void adamw_segment_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, const uint8_t* __restrict__ decay, int64_t n, float lr_seg,
                                                            float wd, float b1, float b2, float eps, float lr_scale,
                                                            const float* __restrict__ scal) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const float coef = scal[0], step_size = scal[1] * lr_scale, inv_sqrt_bc2 = scal[2];
    const int cnt = (int)min((int64_t)4, n - i);
    for (int k = 0; k < cnt; ++k) {
        const int64_t j = i + k;
        const float gg = g[j] * coef;
        float pp = p[j] * (1.f - lr_seg * (decay[j] ? wd : 0.f));
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

int launch_step_prepare(const float* part, int nparts, float max_norm, float lr, float b1, float b2, int64_t* step, float* scal,
                        const LrSchedule& sched, const StepGuard* gd, hipStream_t st) {
    const auto prepare = gd ? adam_prepare_step_kernel<true> : adam_prepare_step_kernel<false>;
    hipLaunchKernelGGL(prepare, dim3(1), dim3(64), 0, st, part, nparts, max_norm, lr, b1, b2, step, scal, sched, gd ? *gd : StepGuard{});
    PMGT_LAUNCH_OK();
    return 0;
}

// adamw_step of csrc/optim.hip: norm partials -> prepare -> AdamW, three launches; gd = NULL: the scheduled form, else the guarded one
static int adamw_step_derived(const AdamArgs& a, const LrSchedule& sched, const StepGuard* gd, hipStream_t st) {
    if (a.n <= 0) return 0;
    const int nparts = (int)std::min<int64_t>(1024, cdiv64(a.n, 1024));
    const auto update = gd ? adamw_step_kernel<true> : adamw_step_kernel<false>;
    hipLaunchKernelGGL(sqnorm_part_kernel, dim3(nparts), dim3(256), 0, st, a.g, a.n, a.part);
    PMGT_LAUNCH_OK();
    if (int rc = launch_step_prepare(a.part, nparts, a.max_norm, a.lr, a.b1, a.b2, a.step, a.scal, sched, gd, st)) return rc;
    hipLaunchKernelGGL(update, dim3((unsigned)cdiv64(cdiv64(a.n, 4), 256)), dim3(256), 0, st, a.p, a.g, a.m, a.v, a.decay, a.n, a.wd, a.b1, a.b2,
                       a.eps, a.scal);
    PMGT_LAUNCH_OK();
    return 0;
}

// null_is_constant: a NULL schedule is the constant rate (lambda = 1, so lr_t = (double)lr and the step is pmgt_optimizer_step's bit for bit)
int schedule_from(const pmgt_lr_schedule* in, bool null_is_constant, float lr, const char* who, LrSchedule* out) {
    if (in == nullptr && null_is_constant) {
        *out = LrSchedule{PMGT_LR_CONSTANT, 0, 0};
        return 0;
    }
    PMGT_CHECK(in != nullptr, -2, "%s: NULL schedule", who);
    const long long W = in->num_warmup_steps, T = in->num_training_steps;
    PMGT_CHECK(in->type >= PMGT_LR_CONSTANT && in->type <= PMGT_LR_POLYNOMIAL, -2, "%s: unknown lr schedule type %d", who, in->type);
    PMGT_CHECK(W >= 0, -2, "%s: num_warmup_steps = %lld is negative", who, W);
    PMGT_CHECK(in->type < PMGT_LR_LINEAR || T > 0, -2, "%s: this lr schedule needs num_training_steps > 0 (got %lld)", who, T);
    if (in->type == PMGT_LR_POLYNOMIAL) {
        PMGT_CHECK((double)lr > 1e-7, -2, "%s: polynomial lr schedule: lr_end (1e-07) must be smaller than the initial lr (%g)", who, (double)lr);
        PMGT_CHECK(T > W, -2, "%s: polynomial lr schedule needs num_training_steps (%lld) > num_warmup_steps (%lld)", who, T, W);
    }
    *out = LrSchedule{in->type, in->num_warmup_steps, in->num_training_steps};
    return 0;
}

int guard_from(const pmgt_step_guard* in, const char* who, StepGuard* out) {
    PMGT_CHECK(in != nullptr, -2, "%s: NULL guard", who);
    PMGT_CHECK(in->counters != nullptr, -2, "%s: NULL guard counters", who);
    PMGT_CHECK(in->log_rows >= 0, -2, "%s: log_rows = %lld is negative", who, (long long)in->log_rows);
    PMGT_CHECK(in->log_rows == 0 || (in->log_f && in->log_i), -2, "%s: log_rows = %lld but a log pointer is NULL", who, (long long)in->log_rows);
    *out = StepGuard{in->counters, in->log_f, in->log_i, in->log_rows, in->loss, in->skip_nonfinite};
    return 0;
}

// the loose argument list of the pmgt_op_adamw* entries is AdamArgs' field order
static AdamArgs adam_args(float* p, const float* g, float* m, float* v, const uint8_t* decay, int64_t n, float lr, float wd, float b1, float b2,
                          float eps, float max_norm, int64_t* step, float* scal, float* part) {
    return AdamArgs{p, g, m, v, decay, n, lr, wd, b1, b2, eps, max_norm, step, scal, part};
}
static bool adam_ptrs_ok(const pmgt_engine* e, const pmgt_tensors* t, const pmgt_adam* a) {
    return e && t && a && t->params && t->grads && a->exp_avg && a->exp_avg_sq && a->decay && a->step && a->scalars && a->scratch;
}
static AdamArgs adam_args(pmgt_engine* e, const pmgt_tensors* t, const pmgt_adam* a) {
    return adam_args(t->params, t->grads, a->exp_avg, a->exp_avg_sq, a->decay, pmgt_param_count(e), a->lr, a->weight_decay, a->beta1, a->beta2,
                     a->eps, a->max_grad_norm, a->step, a->scalars, a->scratch);
}

}  // namespace pmgt

using namespace pmgt;

extern "C" {

int pmgt_optimizer_step_scheduled(pmgt_engine* e, const pmgt_tensors* t, const pmgt_adam* a, const pmgt_lr_schedule* sched, void* stream) {
    PMGT_CHECK(adam_ptrs_ok(e, t, a) && sched, -2, "pmgt_optimizer_step_scheduled: NULL argument");
    LrSchedule s;
    if (int rc = schedule_from(sched, false, a->lr, "pmgt_optimizer_step_scheduled", &s)) return rc;
    return adamw_step_derived(adam_args(e, t, a), s, nullptr, (hipStream_t)stream);
}

int pmgt_optimizer_step_guarded(pmgt_engine* e, const pmgt_tensors* t, const pmgt_adam* a, const pmgt_lr_schedule* sched,
                                const pmgt_step_guard* guard, void* stream) {
    PMGT_CHECK(adam_ptrs_ok(e, t, a), -2, "pmgt_optimizer_step_guarded: NULL argument");
    LrSchedule s;
    if (int rc = schedule_from(sched, true, a->lr, "pmgt_optimizer_step_guarded", &s)) return rc;
    StepGuard gd;
    if (int rc = guard_from(guard, "pmgt_optimizer_step_guarded", &gd)) return rc;
    return adamw_step_derived(adam_args(e, t, a), s, &gd, (hipStream_t)stream);
}

int pmgt_op_adamw(float* p, const float* g, float* m, float* v, const uint8_t* decay, int64_t n, float lr, float wd, float b1, float b2,
                  float eps, float max_norm, int64_t* step, float* scal, float* part, void* stream) {
    return adamw_step(adam_args(p, g, m, v, decay, n, lr, wd, b1, b2, eps, max_norm, step, scal, part), (hipStream_t)stream);
}

int pmgt_op_adamw_scheduled(float* p, const float* g, float* m, float* v, const uint8_t* decay, int64_t n, float lr, float wd, float b1,
                            float b2, float eps, float max_norm, int64_t* step, float* scal, float* part, const pmgt_lr_schedule* sched,
                            void* stream) {
    LrSchedule s;
    if (int rc = schedule_from(sched, false, lr, "pmgt_op_adamw_scheduled", &s)) return rc;
    return adamw_step_derived(adam_args(p, g, m, v, decay, n, lr, wd, b1, b2, eps, max_norm, step, scal, part), s, nullptr, (hipStream_t)stream);
}

int pmgt_op_adamw_guarded(float* p, const float* g, float* m, float* v, const uint8_t* decay, int64_t n, float lr, float wd, float b1,
                          float b2, float eps, float max_norm, int64_t* step, float* scal, float* part, const pmgt_lr_schedule* sched,
                          const pmgt_step_guard* guard, void* stream) {
    LrSchedule s;
    if (int rc = schedule_from(sched, true, lr, "pmgt_op_adamw_guarded", &s)) return rc;
    StepGuard gd;
    if (int rc = guard_from(guard, "pmgt_op_adamw_guarded", &gd)) return rc;
    return adamw_step_derived(adam_args(p, g, m, v, decay, n, lr, wd, b1, b2, eps, max_norm, step, scal, part), s, &gd, (hipStream_t)stream);
}

int pmgt_op_adamw_segments(const pmgt_adam_segment* segments, int count, float lr, float wd, float b1, float b2, float eps, float max_norm,
                           int64_t* step, float* scal, float* part, void* stream) {
    const char* who = "pmgt_op_adamw_segments";
    PMGT_CHECK(count >= 1 && count <= PMGT_ADAM_MAX_SEGMENTS, -2, "%s: %d segments outside [1, %d]", who, count, PMGT_ADAM_MAX_SEGMENTS);
    PMGT_CHECK(segments && step && scal && part, -2, "%s: NULL argument", who);
    SegParts sp = {};
    sp.count = count;
    for (int k = 0; k < count; ++k) {
        const pmgt_adam_segment& s = segments[k];
        PMGT_CHECK(s.n >= 0, -2, "%s: segment %d has n = %lld", who, k, (long long)s.n);
        PMGT_CHECK(s.p && s.g && s.m && s.v && s.decay, -2, "%s: segment %d has a NULL pointer", who, k);
        PMGT_CHECK(std::isfinite(s.lr_scale) && s.lr_scale >= 0.f, -2, "%s: segment %d has lr_scale = %g, not finite or negative", who, k,
                   (double)s.lr_scale);
        sp.nparts[k] = (int)std::min<int64_t>(1024, cdiv64(s.n, 1024));
    }
    const hipStream_t st = (hipStream_t)stream;
    for (int k = 0; k < count; ++k) {
        if (sp.nparts[k] == 0) continue;                     // (an empty segment adds nothing to the norm and steps nothing)
        hipLaunchKernelGGL(sqnorm_part_kernel, dim3(sp.nparts[k]), dim3(256), 0, st, segments[k].g, segments[k].n, part + 1024 * k);
        PMGT_LAUNCH_OK();
    }
    hipLaunchKernelGGL(adam_prepare_segments_kernel, dim3(1), dim3(64), 0, st, part, sp, max_norm, lr, b1, b2, step, scal);
    PMGT_LAUNCH_OK();
    for (int k = 0; k < count; ++k) {
        const pmgt_adam_segment& s = segments[k];
        if (s.n == 0) continue;
        hipLaunchKernelGGL(adamw_segment_kernel, dim3((unsigned)cdiv64(cdiv64(s.n, 4), 256)), dim3(256), 0, st, s.p, s.g, s.m, s.v, s.decay, s.n,
                           lr * s.lr_scale, wd, b1, b2, eps, s.lr_scale, scal);
        PMGT_LAUNCH_OK();
    }
    return 0;
}

int pmgt_op_lr_schedule(const pmgt_lr_schedule* sched, float lr, int64_t first_step, int n, float* out, void* stream) {
    LrSchedule s;
    if (int rc = schedule_from(sched, false, lr, "pmgt_op_lr_schedule", &s)) return rc;
    PMGT_CHECK(out || n <= 0, -2, "pmgt_op_lr_schedule: NULL output");
    if (n <= 0) return 0;
    hipLaunchKernelGGL(lr_schedule_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, (hipStream_t)stream, s, lr, first_step, n, out);
    PMGT_LAUNCH_OK();
    return 0;
}

}  // extern "C"
