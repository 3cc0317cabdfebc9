"""The host yardstick of pmgt_op_sgd and the schedule arithmetic of the pair runs; no GPU.

  * sgd_step_host in fp64 (its own clip, a lambda) follows torch.optim.SGD + clip_grad_norm_ + LambdaLR in fp64 on the CPU over 20 steps to
    1e-12 relative: only the rounding of a few hundred fp64 operations separates them.  That pins the COUPLED decay (on the decayed group
    only), the 1e-6 of the clip, and that the schedule counts completed steps.
  * sgd_step_host in fp32 rounds every product and sum once, in the stated order.
  * pair_schedule_steps against the reference's formula (pmgt/base_trainer.py:71-90 with accumulation_step = 1) on hand-computed cases."""
import numpy as np
import pytest
import torch

from pmgt_amd.pair_train import pair_schedule_steps, pair_trainer_options, sgd_step_host
from pmgt_amd.schedule import lr_lambda

N, STEPS, LR, WD = 257, 20, 0.05, 0.1


@pytest.mark.parametrize("kind", ["linear", "cosine", "constant_with_warmup", "polynomial"])
@pytest.mark.parametrize("max_norm", [0.0, 0.5, 1e6], ids=["off", "active", "inactive"])
def test_fp64_host_step_follows_torch_sgd_with_clip_and_lambda_lr(kind, max_norm):
    rng = np.random.default_rng(5)
    p0, decay = rng.standard_normal(N), rng.random(N) < 0.6
    lam = lr_lambda(kind, 4, STEPS, LR)
    a, b = torch.tensor(p0[decay], requires_grad=True), torch.tensor(p0[~decay], requires_grad=True)      # fp64
    opt = torch.optim.SGD([{"params": [a], "weight_decay": WD}, {"params": [b], "weight_decay": 0.0}], lr=LR)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lam)
    p = p0.copy()
    for s in range(STEPS):
        g = rng.standard_normal(N) * (0.2 + 0.1 * s)
        a.grad, b.grad = torch.tensor(g[decay]), torch.tensor(g[~decay])
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_([a, b], max_norm)
        opt.step()
        sched.step()
        p = sgd_step_host(p, g, decay, wd=WD, dtype=np.float64, max_norm=max_norm, lr=LR, lam=lam, step=s)
        want = np.empty(N)
        want[decay], want[~decay] = a.detach().numpy(), b.detach().numpy()
        assert p.dtype == np.float64 and np.abs(p - want).max() <= 1e-12 * np.abs(want).max(), (s, np.abs(p - want).max())
    assert max_norm != 0.5 or np.sqrt((g * g).sum()) > 0.5      # "active" does clip


def test_fp32_host_step_rounds_every_operation_once_in_order():
    rng = np.random.default_rng(6)
    p, g = rng.standard_normal(1000).astype(np.float32), rng.standard_normal(1000).astype(np.float32)
    decay = (rng.random(1000) < 0.5).astype(np.uint8)
    clip, lr_t, wd = np.float32(0.37), np.float32(0.013), np.float32(0.1)
    got = sgd_step_host(p, g, decay, clip, lr_t, wd)
    want = np.empty_like(p)
    for i in range(len(p)):
        gc = np.float32(g[i] * clip)
        d = np.float32(gc + np.float32(wd * p[i])) if decay[i] else gc
        want[i] = np.float32(p[i] - np.float32(lr_t * d))
    assert got.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    # an element without decay never sees wd; clip 1 and lr_t 0 leave p alone
    assert np.array_equal(sgd_step_host(p, g, np.zeros(1000, np.uint8), 1.0, 0.0, 5.0), p)


def test_pair_schedule_steps_is_the_references_formula():
    # 200 positives, 1 negative each: 400 rows, batch 64 -> 7 steps an epoch (the last one short, 16 rows), 4 epochs
    assert pair_schedule_steps(200, 1, 64, 4, 0.1) == (28, 2)
    assert pair_schedule_steps(200, 1, 64, 4, None) == (28, 0)
    # exactly divisible: no short batch
    assert pair_schedule_steps(128, 3, 64, 3, 0.5) == (24, 12)
    # one row over: one more step an epoch
    assert pair_schedule_steps(129, 3, 64, 3, 0.5) == (27, 13)
    # int() truncates: 0.05 * 9 = 0.45 -> 0
    assert pair_schedule_steps(5, 0, 2, 3, 0.05) == (9, 0)
    # a batch larger than the epoch: one step an epoch
    assert pair_schedule_steps(10, 4, 65536, 60, 0.1) == (60, 6)


def test_pair_trainer_options():
    assert pair_trainer_options("fit_x", 200, 1, 64, 4) == dict(optim="adamw", nonfinite=None, step_log=0)
    assert pair_trainer_options("fit_x", 200, 1, 64, 4, "sgd", "cosine", 0.1, "skip", 8) == dict(
        optim="sgd", nonfinite="skip", step_log=8, scheduler_type="cosine", num_warmup_steps=2, num_training_steps=28)
    with pytest.raises(ValueError, match="without scheduler_type"):
        pair_trainer_options("fit_x", 200, 1, 64, 4, scheduler_warmup=0.1)
