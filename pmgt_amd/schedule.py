"""Learning-rate schedules of the reference's `--scheduler-type` / `--scheduler-warmup` (train.py:38-52): the multipliers of
transformers 4.11.2 `optimization.py` (the version the reference pins) with the defaults `get_scheduler` leaves in place, as closed
forms in Python.  The fused optimizer step evaluates the same forms on the device from its step counter (ops/optimizer_step.h:
scheduled_lr); this file is the host statement of them (`LambdaLR` for the Lightning-style path, expected values for the tests) and
the one place the step counts are derived from the command-line arguments."""
from __future__ import annotations

import math

from ._lib import LR_SCHEDULE_TYPES

LR_END = 1e-7                                    # polynomial: transformers' default lr_end (power 1)
NEEDS_WARMUP = LR_SCHEDULE_TYPES[1:]             # every type but "constant" takes num_warmup_steps
NEEDS_TRAINING_STEPS = LR_SCHEDULE_TYPES[2:]


def lr_lambda(scheduler_type: str, num_warmup_steps: int, num_training_steps: int, lr: float):
    """lambda(s): the multiplier of the base rate `lr` after s completed optimizer steps (LambdaLR's convention)."""
    W, T = int(num_warmup_steps or 0), int(num_training_steps or 0)
    if scheduler_type not in LR_SCHEDULE_TYPES:
        raise ValueError(f"scheduler type {scheduler_type!r}: expected one of {LR_SCHEDULE_TYPES}")
    if W < 0:
        raise ValueError(f"num_warmup_steps = {W} is negative")
    if scheduler_type in NEEDS_TRAINING_STEPS and T <= 0:
        raise ValueError(f"{scheduler_type} requires `num_training_steps`, please provide that argument.")
    if scheduler_type == "polynomial":
        if not lr > LR_END:
            raise ValueError(f"lr_end ({LR_END}) must be be smaller than initial lr ({lr})")
        if T <= W:
            raise ValueError(f"polynomial needs num_training_steps ({T}) > num_warmup_steps ({W})")

    def lam(s: int) -> float:
        if scheduler_type != "constant" and s < W:
            return float(s) / float(max(1, W))
        if scheduler_type in ("constant", "constant_with_warmup"):
            return 1.0
        if scheduler_type == "linear":
            return max(0.0, float(T - s) / float(max(1, T - W)))
        if scheduler_type == "polynomial":
            if s > T:
                return LR_END / lr
            return ((lr - LR_END) * (1 - (s - W) / (T - W)) + LR_END) / lr
        q = float(s - W) / float(max(1, T - W))
        if scheduler_type == "cosine":
            return max(0.0, 0.5 * (1.0 + math.cos(math.pi * q)))
        if q >= 1.0:                             # cosine_with_restarts, one cycle
            return 0.0
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * (q % 1.0))))
    return lam


def scheduler_steps(args):
    """(num_warmup_steps, num_training_steps) from the reference's arguments, with the arithmetic of pmgt/base_trainer.py:71-90:
    T = ceil(len(train_ids) / (train_batch_size * accumulation_step)) * num_epochs, W = int(scheduler_warmup * T) (0 for
    "constant", which takes no warm-up).  `args.train_ids` is the caller's to supply: the reference reads it and never sets it.
    Both get_scheduler and a caller who builds a Trainer from the same `args` take the counts from here."""
    kind = args.scheduler_type
    step_size = args.train_batch_size * args.accumulation_step
    total = (len(args.train_ids) + step_size - 1) // step_size * args.num_epochs
    warmup = getattr(args, "scheduler_warmup", None)
    if warmup is None:
        if kind in NEEDS_WARMUP:
            raise ValueError(f"{kind} requires `num_warmup_steps`, please provide that argument.")
        return 0, total
    return (int(warmup * total) if kind in NEEDS_WARMUP else 0), total
