// pmgt_op_step_segments of include/pmgt_ops.h: up to PMGT_ADAM_MAX_SEGMENTS disjoint flat fp32 buffers stepped as ONE optimizer --
// pmgt_op_adamw_segments (optimizer_step.hip) with the options of the single-buffer entries: a learning-rate schedule evaluated on the device,
// the step guard (a step whose joint gradient norm is not finite is skipped on the device, counted and logged) and SGD.  What an encoder
// fine-tuned through a head needs to run under the reference's --optim / --scheduler-type / --mp-enabled: the encoder's ranges of the
// engine buffer and the head's flat buffer, each at a rate of its own, under one norm, one clip, one counter.
// The launches are pmgt_op_adamw_segments': per non-empty segment one sqnorm_part_kernel of csrc/optim.hip (segment k's partials at
// part + 1024 k, so the joint norm has that entry's bits), ONE prepare lane, per non-empty segment one update.  The lane's body, the schedule
// and the SGD update are optimizer_step.h's, the text pmgt_op_adamw_guarded and pmgt_op_sgd compile: the clip, lr_t, the guard's decision, its
// counters and its log row are theirs bit for bit.  No sync, no allocation, no atomics: capturable.
// Its own file for optimizer_step.hip's reason for being out of csrc/, and so that pmgt_op_adamw_segments -- what the default fine-tune step
// launches -- stays byte for byte what it was.
#include <cmath>

#include "optimizer_step.h"

namespace pmgt {

__global__ void sqnorm_part_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ part);      // csrc/optim.hip

// adam_prepare_step_kernel of optimizer_step.hip over the partials of EVERY segment: a lane adds its partials of segment 0, then of segment 1,
// ..., in fp64 (adam_prepare_segments_kernel's order; ONE segment: adam_prepare_step_kernel's sum in its order); the rest is that kernel's lane.
template <bool Guarded>
__global__ __launch_bounds__(64) void prepare_step_segments_kernel(const float* __restrict__ part, const SegParts sp, float max_norm, float lr,
                                                                   float b1, float b2, int64_t* __restrict__ step, float* __restrict__ scal,
                                                                   const LrSchedule sched, const StepGuard gd) {
    double s = 0.0;
    for (int k = 0; k < sp.count; ++k)
        for (int i = threadIdx.x; i < sp.nparts[k]; i += 64) s += (double)part[k * 1024 + i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (threadIdx.x != 0) return;
    prepare_step_lane<Guarded>(s, max_norm, lr, b1, b2, step, scal, sched, gd);
}

// adamw_segment_kernel of optimizer_step.hip, the same fp32 arithmetic in the same order, with the rate read from the lane: the step size
// is scal[1] * lr_scale and the decay term's rate the fp32 product scal[4] * lr_scale (unscheduled, scal[4] = lr: that kernel's host product).
// Guarded sits behind the skipped flag: scal[5] is one value for the whole grid, so the branch is uniform and a skipped step moves no byte.
template <bool Guarded>
__global__ __launch_bounds__(256) void adamw_step_segment_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                 float* __restrict__ v, const uint8_t* __restrict__ decay, int64_t n, float wd,
                                                                 float b1, float b2, float eps, float lr_scale,
                                                                 const float* __restrict__ scal) {
    if constexpr (Guarded) {
        if (scal[5] != 0.f) return;
    }
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    const float coef = scal[0], step_size = scal[1] * lr_scale, inv_sqrt_bc2 = scal[2], lr_seg = scal[4] * lr_scale;
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

// sgd_update_kernel of sgd_step.hip on one segment: lr_t = scal[4] * lr_scale, ONE rounded fp32 product (lr_scale == 1: that kernel's bits;
// lr_scale == 0 with finite gradients: p - 0 * d = p bit for bit)
template <bool Guarded>
__global__ __launch_bounds__(256) void sgd_step_segment_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                               const uint8_t* __restrict__ decay, int64_t n, int64_t head, int64_t nvec, bool vec,
                                                               bool dec4, float wd, float lr_scale, const float* __restrict__ scal) {
    if constexpr (Guarded) {
        if (scal[5] != 0.f) return;
    }
    sgd_update_range(p, g, decay, n, head, nvec, vec, dec4, wd, scal[0], scal[4] * lr_scale);
}

}  // namespace pmgt

using namespace pmgt;

extern "C" int pmgt_op_step_segments(const pmgt_adam_segment* segments, int count, int optim, float lr, float wd, float b1, float b2, float eps,
                                     float max_norm, int64_t* step, float* scal, float* part, const pmgt_lr_schedule* sched,
                                     const pmgt_step_guard* guard, void* stream) {
    const char* who = "pmgt_op_step_segments";
    PMGT_CHECK(count >= 1 && count <= PMGT_ADAM_MAX_SEGMENTS, -2, "%s: %d segments outside [1, %d]", who, count, PMGT_ADAM_MAX_SEGMENTS);
    PMGT_CHECK(segments && step && scal && part, -2, "%s: NULL argument", who);
    PMGT_CHECK(optim == PMGT_OPTIM_ADAMW || optim == PMGT_OPTIM_SGD, -2, "%s: optim = %d is neither PMGT_OPTIM_ADAMW nor PMGT_OPTIM_SGD", who, optim);
    PMGT_CHECK(std::isfinite(lr) && std::isfinite(wd) && std::isfinite(max_norm), -2, "%s: lr = %g, wd = %g or max_norm = %g is not finite", who,
               (double)lr, (double)wd, (double)max_norm);
    const bool sgd = optim == PMGT_OPTIM_SGD;
    SegParts sp = {};
    sp.count = count;
    for (int k = 0; k < count; ++k) {
        const pmgt_adam_segment& s = segments[k];
        PMGT_CHECK(s.n >= 0, -2, "%s: segment %d has n = %lld", who, k, (long long)s.n);
        PMGT_CHECK(s.p && s.g && s.decay && (sgd || (s.m && s.v)), -2, "%s: segment %d has a NULL pointer", who, k);
        PMGT_CHECK(std::isfinite(s.lr_scale) && s.lr_scale >= 0.f, -2, "%s: segment %d has lr_scale = %g, not finite or negative", who, k,
                   (double)s.lr_scale);
        sp.nparts[k] = (int)std::min<int64_t>(1024, cdiv64(s.n, 1024));
    }
    LrSchedule sc;
    if (int rc = schedule_from(sched, true, lr, who, &sc)) return rc;
    StepGuard gd = {};
    if (guard != nullptr)
        if (int rc = guard_from(guard, who, &gd)) return rc;
    const hipStream_t st = (hipStream_t)stream;
    for (int k = 0; k < count; ++k) {
        if (sp.nparts[k] == 0) continue;                     // (an empty segment adds nothing to the norm and steps nothing)
        hipLaunchKernelGGL(sqnorm_part_kernel, dim3(sp.nparts[k]), dim3(256), 0, st, segments[k].g, segments[k].n, part + 1024 * k);
        PMGT_LAUNCH_OK();
    }
    // SGD: beta1 = beta2 = 0 as pmgt_op_sgd passes them: the bias corrections are 1 exactly, scal[1] = lr_t and scal[2] = 1
    const auto prepare = guard ? prepare_step_segments_kernel<true> : prepare_step_segments_kernel<false>;
    hipLaunchKernelGGL(prepare, dim3(1), dim3(64), 0, st, part, sp, max_norm, lr, sgd ? 0.f : b1, sgd ? 0.f : b2, step, scal, sc, gd);
    PMGT_LAUNCH_OK();
    for (int k = 0; k < count; ++k) {
        const pmgt_adam_segment& s = segments[k];
        if (s.n == 0) continue;
        if (sgd) {
            const SgdSplit sg = sgd_split(s.p, s.g, s.decay, s.n);
            const auto update = guard ? sgd_step_segment_kernel<true> : sgd_step_segment_kernel<false>;
            hipLaunchKernelGGL(update, dim3(sg.blocks), dim3(256), 0, st, s.p, s.g, s.decay, s.n, sg.head, sg.nvec, sg.vec, sg.dec4, wd, s.lr_scale,
                               scal);
        } else {
            const auto update = guard ? adamw_step_segment_kernel<true> : adamw_step_segment_kernel<false>;
            hipLaunchKernelGGL(update, dim3((unsigned)cdiv64(cdiv64(s.n, 4), 256)), dim3(256), 0, st, s.p, s.g, s.m, s.v, s.decay, s.n, wd, b1, b2,
                               eps, s.lr_scale, scal);
        }
        PMGT_LAUNCH_OK();
    }
    return 0;
}
