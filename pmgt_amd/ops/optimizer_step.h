// What the optimizer entries outside csrc/ share (optimizer_step.hip defines it; sgd_step.hip is the other user): the checked forms of
// pmgt_lr_schedule and pmgt_step_guard, and the launch of the ONE prepare lane, so that every entry evaluates the schedule, the clip and the
// guard with the same device code and therefore the same bits.
#pragma once
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

// null_is_constant: a NULL schedule is the constant rate (lambda = 1, so lr_t = (double)lr and the step is pmgt_optimizer_step's bit for bit)
int schedule_from(const pmgt_lr_schedule* in, bool null_is_constant, float lr, const char* who, LrSchedule* out);
int guard_from(const pmgt_step_guard* in, const char* who, StepGuard* out);
// one launch of the prepare lane over `nparts` partials of sqnorm_part_kernel (0: the norm is 0); gd = NULL: unguarded
int launch_step_prepare(const float* part, int nparts, float max_norm, float lr, float b1, float b2, int64_t* step, float* scal,
                        const LrSchedule& sched, const StepGuard* gd, hipStream_t st);

}  // namespace pmgt
