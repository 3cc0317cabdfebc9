// What the optimizer entries outside csrc/ share (optimizer_step.hip defines the host side; sgd_step.hip and segments_step.hip are the other
// users): the checked forms of pmgt_lr_schedule and pmgt_step_guard, the launch of the ONE prepare lane, and -- as device code every user
// compiles from this one text -- the schedule, the lane's body and the SGD update, so that every entry evaluates the schedule, the clip, the
// guard and the SGD element with the same device code and therefore the same bits.
#pragma once
#include <cmath>

#include "../../include/pmgt_ops.h"
#include "../csrc/common.h"

namespace pmgt {

struct LrSchedule {
    int type;                  // PMGT_LR_*
    int64_t warmup, total;     // num_warmup_steps (W), num_training_steps (T)
};

struct StepGuard {
    int64_t* counters;      // [4]: attempts, skipped, skipped in a row, reserved
    float* log_f;           // [log_rows][PMGT_STEP_LOG_FLOATS] or NULL
    int64_t* log_i;         // [log_rows][2] or NULL
    int64_t log_rows;
    const float* loss;      // device scalar or NULL
    int skip_nonfinite;
};

// several flat buffers as ONE optimizer: the partials of segment s are sqnorm_part_kernel's, nparts[s] of them at part + 1024 s
struct SegParts {
    int count;
    int nparts[PMGT_ADAM_MAX_SEGMENTS];
};

// null_is_constant: a NULL schedule is the constant rate (lambda = 1, so lr_t = (double)lr and the step is pmgt_optimizer_step's bit for bit)
int schedule_from(const pmgt_lr_schedule* in, bool null_is_constant, float lr, const char* who, LrSchedule* out);
int guard_from(const pmgt_step_guard* in, const char* who, StepGuard* out);
// one launch of the prepare lane over `nparts` partials of sqnorm_part_kernel (0: the norm is 0); gd = NULL: unguarded
int launch_step_prepare(const float* part, int nparts, float max_norm, float lr, float b1, float b2, int64_t* step, float* scal,
                        const LrSchedule& sched, const StepGuard* gd, hipStream_t st);

// lr * lambda(s): LambdaLR's rate after s completed optimizer steps
static __device__ double scheduled_lr(const LrSchedule sc, double lr, int64_t s) {
    const double W = (double)sc.warmup, T = (double)sc.total, x = (double)s;
    if (sc.type != PMGT_LR_CONSTANT && s < sc.warmup) return lr * (x / fmax(1.0, W));
    const double q = (x - W) / fmax(1.0, T - W);
    switch (sc.type) {
        case PMGT_LR_LINEAR: return lr * fmax(0.0, (T - x) / fmax(1.0, T - W));
        case PMGT_LR_COSINE: return lr * fmax(0.0, 0.5 * (1.0 + cos(M_PI * q)));                                  // half a cycle
        case PMGT_LR_COSINE_WITH_RESTARTS: return q >= 1.0 ? 0.0 : lr * fmax(0.0, 0.5 * (1.0 + cos(M_PI * fmod(q, 1.0))));      // one cycle
        case PMGT_LR_POLYNOMIAL: return lr * ((s > sc.total ? 1e-7 : (lr - 1e-7) * (1.0 - (x - W) / (T - W)) + 1e-7) / lr);    // power 1, lr_end 1e-7
        default: return lr;                                                                                      // constant, constant_with_warmup
    }
}

// The body of the prepare lane, run by ONE thread on `s`, the fp64 sum of the norm partials over the wave: adam_prepare_kernel of
// csrc/optim.hip with lr_t for lr: fp64, rounded once per slot.  Guarded adds the decision, the counters and the log row; a skipped step
// leaves step[0], scal[1] and scal[2] alone (the bias corrections and the schedule count applied steps only) and reports the rate it would
// have used.  The unguarded form neither reads nor writes scal[5..7], nor gd.
template <bool Guarded>
static __device__ __forceinline__ void prepare_step_lane(double s, float max_norm, float lr, float b1, float b2, int64_t* __restrict__ step,
                                                         float* __restrict__ scal, const LrSchedule& sched, const StepGuard& gd) {
    const double norm = sqrt(s);
    bool bad = false, skip = false;
    if constexpr (Guarded) {
        bad = !isfinite(norm);
        skip = bad && gd.skip_nonfinite != 0;
    }
    int64_t t = step[0];
    double coef = 0.0, lr_t;
    if (skip) {
        lr_t = scheduled_lr(sched, (double)lr, t);
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
    if constexpr (Guarded) {
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

// ---- the SGD update (pmgt_op_sgd; pmgt_op_step_segments per segment).  Compiled WITHOUT contraction: every product and sum is rounded to fp32
// in the order written, which is what lets a numpy fp32 restatement (pair_train.sgd_step_host) agree bit for bit.
static __device__ __forceinline__ float sgd_element(float p, float g, bool decays, float clip, float lr_t, float wd) {
#pragma clang fp contract(off)
    const float gc = g * clip;
    const float d = decays ? gc + wd * p : gc;
    return p - lr_t * d;
}

// How a launch walks p [n]: head = the floats in front of the first 16-byte boundary of p (0..3, at most n); the body is nvec whole f32x4 from
// there; the tail is what is left (0..3).  vec: g shares p's alignment (the body moves 16 bytes a lane; else element by element); dec4: the
// body's decay bytes can be read 4 at a time.  blocks: 8 blocks a CU on 256 CUs keep HBM busy; beyond that the grid strides.
struct SgdSplit {
    int64_t head, nvec;
    bool vec, dec4;
    unsigned blocks;
};

static inline SgdSplit sgd_split(const float* p, const float* g, const uint8_t* decay, int64_t n) {
    SgdSplit sp;
    sp.head = std::min<int64_t>(n, (int64_t)(((16 - ((uintptr_t)p & 15)) & 15) / 4));
    sp.nvec = (n - sp.head) / 4;
    sp.vec = ((uintptr_t)(p + sp.head) & 15) == 0 && ((uintptr_t)(g + sp.head) & 15) == 0;
    sp.dec4 = ((uintptr_t)(decay + sp.head) & 3) == 0;
    sp.blocks = (unsigned)std::min<int64_t>(2048, std::max<int64_t>(1, cdiv64(sp.nvec, 256)));
    return sp;
}

// One grid of 256-lane blocks over an SgdSplit: the body grid-stride; head and tail are block 0's, one lane an element.  The element-by-element
// body is a CORRECTNESS fallback (strided 4-byte accesses; nothing times it): the trainers' parameters and gradients are whole allocations, or
// views at the same offset of both, and take the 16-byte body.
static __device__ __forceinline__ void sgd_update_range(float* __restrict__ p, const float* __restrict__ g, const uint8_t* __restrict__ decay,
                                                        int64_t n, int64_t head, int64_t nvec, bool vec, bool dec4, float wd, float clip,
                                                        float lr_t) {
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
