// The learning-rate schedule as the device evaluates it, shared by the scheduled step (lr_schedule.hip) and the guarded step
// (guarded_step.hip): the descriptor handed to a kernel by value, lr * lambda(s), and the argument checks of pmgt_lr_schedule.
#pragma once
#include "../../include/pmgt_ops.h"
#include "../csrc/optim.h"

namespace pmgt {

struct LrSchedule {
    int type;                  // PMGT_LR_*
    int64_t warmup, total;     // num_warmup_steps (W), num_training_steps (T)
};

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

static inline int schedule_from(const pmgt_lr_schedule* in, float lr, const char* who, LrSchedule* out) {
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

}  // namespace pmgt
