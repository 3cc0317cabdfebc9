"""Learning-rate schedules evaluated on the device (pmgt_amd/ops/optimizer_step.hip: scheduled_lr and the unguarded instantiation of
adam_prepare_step_kernel / adamw_step_kernel), from the single-kernel entries up to captured trainer steps.  Expected values: the closed forms of transformers 4.11.2
in float64 (tests/lr_schedule_util.py); the reference's own get_scheduler cannot run, so no fixture comes from it.

Bounds.  A rate: one fp32 ulp of float32(lr * lambda(s)) plus 1e-12 lr -- the device evaluates in double, its cos differs from the
host's by a few double ulps, and one rounding to fp32 follows; the absolute term covers the zeros of the cosine.  The optimizer step:
those of test_clip_and_adamw_three_steps (tests/test_rowops_gpu.py).  Captured against eager: bit-identical."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import golden_util as gu
from tests import lr_schedule_util as su
from tests.test_engine_gpu import dev_batch, make_engine
from tests.test_rowops_gpu import ADAM, H, P, assert_close, check, nans, stream, ulp

pytestmark = pytest.mark.gpu

LR = ADAM["lr"]          # 1e-3 as the kernel receives it (rounded to fp32)


def _sched(kind, W, T):
    from pmgt_amd import _lib
    return _lib.LrScheduleC(su.TYPES.index(kind), W, T)


def _device_curve(kind, W, T, lr, first, n):
    out = nans((n + 3,))
    sc = _sched(kind, W, T)
    check(H().pmgt_op_lr_schedule(C.byref(sc), lr, first, n, P(out), stream()))
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[n:]).all())          # nothing written past n
    return out[:n].cpu().numpy()


# every type at every (W, T), (10, 10) and (0, 1) being the degenerate ones; polynomial with T <= W is refused (transformers divides
# by zero there): test_bad_schedules_are_refused
CURVES = [(k, W, T) for W, T in [(0, 10), (3, 10), (1000, 100000), (10, 10), (0, 1)] for k in su.TYPES
          if not (k == "polynomial" and T <= W)]


@pytest.mark.parametrize("kind,W,T", CURVES)
def test_device_curve_equals_the_closed_form(kind, W, T):
    got = _device_curve(kind, W, T, LR, 0, T + 6)
    su.assert_on_curve(got, su.curve(kind, W, T, LR, range(T + 6)), LR, what=(kind, W, T))
    if kind != "constant" and W > 0:
        assert got[0] == 0.0
    # a window that does not start at 0, and another base rate
    got = _device_curve(kind, W, T, 0.25, max(T - 3, 0), 7)
    su.assert_on_curve(got, su.curve(kind, W, T, 0.25, range(max(T - 3, 0), max(T - 3, 0) + 7)), 0.25, what=(kind, W, T, "window"))


def test_bad_schedules_are_refused():
    from pmgt_amd import _lib
    out = nans((4,))

    def refused(sc, lr, text):
        assert H().pmgt_op_lr_schedule(C.byref(sc), lr, 0, 4, P(out), stream()) == -2
        assert text in H().pmgt_last_error().decode()
    refused(_lib.LrScheduleC(6, 0, 10), LR, "unknown")
    refused(_lib.LrScheduleC(-1, 0, 10), LR, "unknown")
    refused(_sched("linear", -1, 10), LR, "num_warmup_steps")
    for kind in su.TYPES[2:]:
        refused(_sched(kind, 0, 0), LR, "num_training_steps")
    refused(_sched("polynomial", 0, 10), 5e-8, "lr_end")
    refused(_sched("polynomial", 10, 10), LR, "num_warmup_steps")
    refused(_sched("polynomial", 11, 10), LR, "num_warmup_steps")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    sc = _sched("constant", 0, 0)           # the two constant types need no num_training_steps
    check(H().pmgt_op_lr_schedule(C.byref(sc), LR, 0, 4, P(out), stream()))
    torch.cuda.synchronize()
    assert out.tolist() == [LR] * 4


def _adamw_scheduled(p, g, m, v, dec, n, max_norm, step, scal, part, sc):
    a = ADAM
    check(H().pmgt_op_adamw_scheduled(P(p), P(g), P(m), P(v), P(dec), n, a["lr"], a["wd"], a["b1"], a["b2"], a["eps"], max_norm, P(step),
                                      P(scal), P(part), C.byref(sc), stream()))


@pytest.mark.parametrize("n", [5, 4095, (1 << 20) + 3])
def test_scheduled_adamw_six_steps_of_a_linear_schedule(n):
    """linear, W = 2, T = 5: lambda = 0, 1/2, 1, 2/3, 1/3, 0 -- step 0 and the clamp past T leave p untouched while step, m and v advance.
    fp64 restatement and bounds of test_clip_and_adamw_three_steps, with lr_t in the step size and in the decay term."""
    a = ADAM
    W, T = 2, 5
    sc = _sched("linear", W, T)
    gen = torch.Generator(device="cuda").manual_seed(n)
    p = torch.randn(n, device="cuda", generator=gen)
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    dec = (torch.rand(n, device="cuda", generator=gen) < 0.6).to(torch.uint8)
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    scal, part = nans((8,)), nans((1024,))
    for t in range(1, 7):
        g = torch.randn(n, device="cuda", generator=gen) * (0.5 * t)
        norm = float(g.double().norm())
        max_norm = 0.01 * norm if t % 2 else 0.0
        p_in = p.clone()
        p0, m0, v0 = p.double(), m.double(), v.double()
        _adamw_scheduled(p, g, m, v, dec, n, max_norm, step, scal, part, sc)
        torch.cuda.synchronize()
        lr_t = a["lr"] * su.lam("linear", W, T, a["lr"], t - 1)
        assert (lr_t == 0) == (t in (1, 6)) and (lr_t == a["lr"]) == (t == 3)
        coef = min(max_norm / (norm + 1e-6), 1.0) if max_norm > 0 else 1.0
        bc1, bc2 = 1 - a["b1"] ** t, 1 - a["b2"] ** t
        assert int(step[0]) == t
        sc_ = scal.cpu().double()
        assert abs(float(sc_[3]) - norm) <= 1e-5 * norm
        assert abs(float(sc_[0]) - coef) <= 1e-5 * coef
        assert abs(float(sc_[1]) - lr_t / bc1) <= 1e-6 * lr_t / bc1
        assert abs(float(sc_[2]) - 1 / math.sqrt(bc2)) <= 1e-6 / math.sqrt(bc2)
        su.assert_on_curve(float(sc_[4]), lr_t, a["lr"], what=f"scal[4] (step {t})")
        assert bool(torch.isnan(scal[5:]).all())                      # slots 5 - 7 are not the kernel's
        gg = g.double() * float(sc_[0])
        m_ref = a["b1"] * m0 + (1 - a["b1"]) * gg
        v_ref = a["b2"] * v0 + (1 - a["b2"]) * gg * gg
        p_ref = p0 * (1 - lr_t * a["wd"] * dec.double()) - (lr_t / bc1) * m_ref / (v_ref.sqrt() / math.sqrt(bc2) + a["eps"])
        assert_close(m, m_ref, torch.float32, ulps=16, floor=1e-7, what=f"m (step {t})")
        assert_close(v, v_ref, torch.float32, ulps=16, floor=1e-7, what=f"v (step {t})")
        err = (p.double() - p_ref).abs()
        bound = 2 * ulp(p_ref, torch.float32) + 1e-3 * lr_t
        assert bool((err <= bound).all()), f"p (step {t}): max error {float(err.max())!r}, {int((err > bound).sum())} elements out of bound"
        if lr_t == 0:
            assert float(sc_[4]) == 0.0 and float(sc_[1]) == 0.0
            assert torch.equal(p, p_in)                               # bit-identical
            assert not torch.equal(m.double(), m0) and not torch.equal(v.double(), v0)
        else:
            assert not torch.equal(p, p_in)


@pytest.mark.parametrize("n", [3, 4095, (1 << 20) + 3])
def test_constant_schedule_is_bit_identical_to_the_unscheduled_step(n):
    """lr * 1.0 is exact: type `constant` through the scheduled entry gives the p, m, v of pmgt_op_adamw, over 3 steps"""
    a = ADAM
    gen = torch.Generator(device="cuda").manual_seed(n + 7)
    p0 = torch.randn(n, device="cuda", generator=gen)
    dec = (torch.rand(n, device="cuda", generator=gen) < 0.6).to(torch.uint8)
    gs = [torch.randn(n, device="cuda", generator=gen) * (0.5 * t) for t in (1, 2, 3)]
    res = []
    for scheduled in (False, True):
        p, m, v = p0.clone(), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
        step = torch.zeros(1, dtype=torch.int64, device="cuda")
        scal, part = nans((8 if scheduled else 4,)), nans((1024,))
        sc = _sched("constant", 0, 0)
        for g in gs:
            if scheduled:
                _adamw_scheduled(p, g, m, v, dec, n, 1.0, step, scal, part, sc)
            else:
                check(H().pmgt_op_adamw(P(p), P(g), P(m), P(v), P(dec), n, a["lr"], a["wd"], a["b1"], a["b2"], a["eps"], 1.0, P(step),
                                        P(scal), P(part), stream()))
        torch.cuda.synchronize()
        assert int(step[0]) == 3
        res.append((p, m, v, scal[:4].clone()))
        if scheduled:
            assert float(scal[4]) == a["lr"] and bool(torch.isnan(scal[5:]).all())
    for x, y in zip(*res):
        assert torch.equal(x, y)


# =========================================================================================== trainer level (golden-sized model m3)
@pytest.fixture(autouse=True)
def _no_graph_left_behind():
    """Captured steps are destroyed HERE, with the GPU idle: a trainer that ran run_live(graphs=True) is cyclic garbage (trainer -> replays
    -> trainer), and a collection that destroyed its graphs and its engine in the middle of a later test's capture would be that test's
    problem."""
    yield
    import gc
    torch.cuda.synchronize()
    gc.collect()


def _trainer(case, dtype, **kw):
    from pmgt_amd.trainer import Trainer
    eng = make_engine(case, dtype=dtype, hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    return eng, Trainer(eng, lr=1e-3, weight_decay=1e-2, max_grad_norm=5.0, **kw)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_captured_steps_follow_the_schedule_and_equal_eager_steps(dtype):
    """linear, W = 2, T = 8: 8 eager steps against 2 warm-up steps + a capture (records, does not run) + 6 replays.  Parameters and both
    moments bit-identical; the rate read back after every replay follows the curve (it is not the capture's)."""
    case = gu.model_case("m3")
    batch = dev_batch(case["batch"])
    kw = dict(scheduler_type="linear", num_warmup_steps=2, num_training_steps=8)
    want = su.curve("linear", 2, 8, float(np.float32(1e-3)), range(8))
    eng_a, tr_a = _trainer(case, dtype, **kw)
    lrs_a = []
    for _ in range(8):
        tr_a.train_step(batch)
        lrs_a.append(eng_a.last_lr().item())
    torch.cuda.synchronize()
    eng_b, tr_b = _trainer(case, dtype, **kw)
    replay = tr_b.capture_step(batch, warmup=2)
    lrs_b = []
    for _ in range(6):
        replay()
        lrs_b.append(eng_b.last_lr().item())
    torch.cuda.synchronize()
    assert int(eng_a.opt_step.item()) == 8 and int(eng_b.opt_step.item()) == 8
    su.assert_on_curve(lrs_a, want, 1e-3, what="eager")
    su.assert_on_curve(lrs_b, want[2:], 1e-3, what="replays")
    assert len(set(lrs_b)) == 6                                   # not one frozen rate
    assert torch.equal(eng_a.params, eng_b.params)
    assert torch.equal(eng_a.exp_avg, eng_b.exp_avg) and torch.equal(eng_a.exp_avg_sq, eng_b.exp_avg_sq)
    # the schedule moved the parameters: a constant-lr trainer ends elsewhere
    eng_c, tr_c = _trainer(case, dtype)
    for _ in range(8):
        tr_c.train_step(batch)
    torch.cuda.synchronize()
    assert not torch.equal(eng_a.params, eng_c.params)


def _live(case):
    from pmgt_amd.datasets import MCNSampler
    from pmgt_amd.graph import synthetic_graph
    n = case["n_nodes"]
    S = case["batch"][0]["node_ids"].shape[1]
    return MCNSampler(synthetic_graph(n, 5 * n, seed=3), S - 1), np.arange(2, n + 2)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_run_live_graphs_follows_a_cosine_schedule_without_recapture(dtype, monkeypatch):
    from pmgt_amd.trainer import Trainer
    case = gu.model_case("m3")
    smp, ids = _live(case)
    lr32 = float(np.float32(1e-3))
    eng, tr = _trainer(case, dtype, scheduler_type="cosine", num_warmup_steps=4, num_training_steps=40)
    captures = []
    orig = Trainer.capture_step
    monkeypatch.setattr(Trainer, "capture_step", lambda self, *a, **k: (captures.append(1), orig(self, *a, **k))[1])
    tr.run_live(smp, ids, batch_size=32, steps=40, threads=3, depth=3, graphs=True)
    torch.cuda.synchronize()
    assert len(tr._live_replays) == 3 and len(captures) == 3      # one capture per slot, none as the rate moved
    taken = int(eng.opt_step.item())
    assert taken == 40
    su.assert_on_curve(eng.last_lr().item(), su.curve("cosine", 4, 40, lr32, [taken - 1]), 1e-3, what="after 40 steps")
    old = set(tr._live_replays)
    tr.num_training_steps = 80                                    # another schedule: the key changes, the slots are captured again
    tr.run_live(smp, ids, batch_size=32, steps=4, threads=3, depth=3, graphs=True)
    torch.cuda.synchronize()
    assert len(captures) == 6 and not (old & set(tr._live_replays))
    taken = int(eng.opt_step.item())
    assert taken == 44
    su.assert_on_curve(eng.last_lr().item(), su.curve("cosine", 4, 80, lr32, [taken - 1]), 1e-3, what="after the change")
    tr.drop_captured_steps()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_schedule_counts_optimizer_steps_and_resumes_from_the_device_counter(dtype):
    case = gu.model_case("m3")
    batch = dev_batch(case["batch"])
    lr32 = float(np.float32(1e-3))
    eng, tr = _trainer(case, dtype, accumulate_grad_batches=2, scheduler_type="linear", num_warmup_steps=4, num_training_steps=10)
    for _ in range(6):
        tr.train_step(batch)
    torch.cuda.synchronize()
    assert int(eng.opt_step.item()) == 3                          # 6 micro-batches = 3 optimizer steps: the last one used lambda(2)
    su.assert_on_curve(eng.last_lr().item(), su.curve("linear", 4, 10, lr32, [2]), 1e-3, what="accumulation")
    eng.opt_step.fill_(7)                                         # a resume: Adam's step count and the schedule move together
    tr.train_step(batch)
    tr.train_step(batch)
    torch.cuda.synchronize()
    assert int(eng.opt_step.item()) == 8
    su.assert_on_curve(eng.last_lr().item(), su.curve("linear", 4, 10, lr32, [7]), 1e-3, what="resume")
    assert eng.grad_norm().item() > 0                             # the norm slot is the same buffer's
