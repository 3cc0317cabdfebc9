"""pmgt_op_sgd alone: fused clip + SGD (no momentum, coupled weight decay) over a flat buffer, optionally scheduled and guarded.

Sizes: a lone element, a body-less tail, one side and the other of a block (1023 / 1025 floats = 255.75 / 256.25 lanes of four) and of a
partials slot (1024 floats each), several partials (4099), 2^20 + 3 (every one of the 1 024 partials strides; the update's 1 024 blocks run
their loop once) and STRIDED = 2^21 + 2^12 + 3: 525 312 groups of four over the update's cap of 2 048 x 256 = 524 288 lanes, so the first
1 024 lanes take the grid-stride loop a SECOND time (aligned, and one float into the allocations), as every step at table sizes does.
The body for `g` aligned differently from `p` (element by element; a correctness fallback that nothing times: the trainers' buffers are
whole allocations) runs at n = 3 (the head is all of it), 4 099 and STRIDED.
  * p equals pair_train.sgd_step_host given the device's scal[0] and scal[4] BIT FOR BIT; scal[3] and scal[0] within the 1e-5 relative bound
    tests/test_adamw_segments_gpu.py holds the AdamW entries to, against an fp64 norm; *step advances by one; g and decay are untouched.
  * Scheduled: scal[4] is pmgt_op_lr_schedule's value bit for bit at steps 0, W - 1, W, T and T + 1 of every schedule type.
  * Guarded: non-finite GRADIENTS (one Inf, one NaN, finite squares that overflow fp32) skip the step; skip_nonfinite = 0 applies and logs.
  * The refusals return -2 and launch nothing."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.pair_train import sgd_step_host
from tests.test_rowops_gpu import P, nans, stream

pytestmark = pytest.mark.gpu

LR, WD = float(np.float32(0.05)), float(np.float32(0.1))
STRIDED = (1 << 21) + (1 << 12) + 3      # more groups of four than the update kernel's 2 048 x 256 lanes: the loop strides
SIZES = [1, 3, 1023, 1025, 4099, (1 << 20) + 3, STRIDED]


def bits(t):
    return t.view(torch.int32)


def make(n, offset=0, seed=None):
    """p, g as views `offset` floats into their allocations, a mixed decay mask, the step counter, scal (NaN), part (NaN)"""
    gen = torch.Generator(device="cuda").manual_seed(n if seed is None else seed)
    p = torch.randn(n + offset, device="cuda", generator=gen)[offset:]
    g = torch.randn(n + offset, device="cuda", generator=gen)[offset:]
    dec = (torch.rand(n, device="cuda", generator=gen) < 0.6).to(torch.uint8)
    return p, g, dec, torch.zeros(1, dtype=torch.int64, device="cuda"), nans((8,)), nans((1024,))


def sgd(p, g, dec, n, max_norm, step, scal, part, sched=None, guard=None, lr=LR, wd=WD):
    return _lib.hip().pmgt_op_sgd(P(p), P(g), P(dec), n, lr, wd, max_norm, P(step), P(scal), P(part),
                                  None if sched is None else C.byref(sched), None if guard is None else C.byref(guard), stream())


def check_applied(p0, g, dec, p, scal, max_norm):
    """the norm and the clip against fp64, p against the fp32 host restatement with the device's clip and rate"""
    sc = scal.cpu()
    norm = float(g.double().norm())
    coef = min(max_norm / (norm + 1e-6), 1.0) if max_norm > 0 else 1.0
    assert abs(float(sc[3]) - norm) <= 1e-5 * norm and abs(float(sc[0]) - coef) <= 1e-5 * coef, (float(sc[3]), norm, float(sc[0]), coef)
    want = sgd_step_host(p0.cpu().numpy(), g.cpu().numpy(), dec.cpu().numpy(), sc[0].numpy(), sc[4].numpy(), np.float32(WD))
    assert np.array_equal(p.cpu().numpy().view(np.int32), want.view(np.int32))
    return sc


@pytest.mark.parametrize("mode", ["off", "inactive", "active"])
@pytest.mark.parametrize("n,offset", [(n, 0) for n in SIZES] + [(4099, 1), (STRIDED, 1)], ids=lambda v: str(v))
def test_sgd_is_the_host_restatement_bit_for_bit(n, offset, mode):
    p, g, dec, step, scal, part = make(n, offset)
    assert offset == 0 or (p.data_ptr() % 16 == 4 and g.data_ptr() % 16 == 4)
    assert n != STRIDED or (n - (3 if offset else 0)) // 4 > 2048 * 256      # the update's grid cannot hold a lane per group
    norm = float(g.double().norm())
    max_norm = {"off": 0.0, "inactive": 10.0 * norm + 1.0, "active": 0.01 * norm}[mode]
    p0, g0, dec0 = p.clone(), g.clone(), dec.clone()
    _lib.check(sgd(p, g, dec, n, max_norm, step, scal, part))
    torch.cuda.synchronize()
    sc = check_applied(p0, g, dec, p, scal, max_norm)
    assert (float(sc[0]) < 0.02) if mode == "active" else float(sc[0]) == 1.0
    assert float(sc[1]) == float(sc[4]) == LR and float(sc[2]) == 1.0 and bool(torch.isnan(sc[5:]).all())      # unguarded: [5..7] untouched
    assert int(step[0]) == 1
    assert torch.equal(bits(g), bits(g0)) and torch.equal(dec, dec0)
    assert not torch.equal(p, p0)


@pytest.mark.parametrize("n", [3, 4099, STRIDED])
def test_g_aligned_differently_from_p_takes_the_element_by_element_body(n):
    """p one float into its allocation, g two: no 16-byte group of p is one of g, so the body runs element by element (strided too at
    STRIDED; at n = 3 the head is everything).  Two steps, the second from the device's own state."""
    p, _, dec, step, scal, part = make(n, 1)
    assert p.data_ptr() % 16 == 4
    for t in (1, 2):
        g = torch.randn(n + 2, device="cuda")[2:]
        assert g.data_ptr() % 16 == 8
        p0, g0 = p.clone(), g.clone()
        max_norm = 0.5 * float(g.double().norm())
        _lib.check(sgd(p, g, dec, n, max_norm, step, scal, part))
        torch.cuda.synchronize()
        check_applied(p0, g, dec, p, scal, max_norm)
        assert int(step[0]) == t and torch.equal(bits(g), bits(g0)) and not torch.equal(p, p0)


def test_zero_elements_run_the_prepare_lane_alone():
    p, g, dec, step, scal, part = make(4)
    p0 = p.clone()
    _lib.check(sgd(p, g, dec, 0, 1.0, step, scal, part))
    torch.cuda.synchronize()
    assert int(step[0]) == 1 and float(scal[3]) == 0.0 and float(scal[0]) == 1.0 and float(scal[4]) == LR and torch.equal(p, p0)


@pytest.mark.parametrize("kind", _lib.LR_SCHEDULE_TYPES)
def test_scheduled_rate_is_pmgt_op_lr_schedule_bit_for_bit(kind):
    W, T, n = 5, 40, 1025
    sched = _lib.LrScheduleC(_lib.LR_SCHEDULE_TYPES.index(kind), W, T)
    want = torch.zeros(1, device="cuda")
    p, g, dec, step, scal, part = make(n)
    for s in (0, W - 1, W, T, T + 1):
        step.fill_(s)
        p0 = p.clone()
        _lib.check(_lib.hip().pmgt_op_lr_schedule(C.byref(sched), LR, s, 1, P(want), stream()))
        _lib.check(sgd(p, g, dec, n, 0.0, step, scal, part, sched=sched))
        torch.cuda.synchronize()
        assert torch.equal(bits(scal[4:5]), bits(want)) and torch.equal(bits(scal[1:2]), bits(want)), (kind, s, float(scal[4]), float(want))
        assert int(step[0]) == s + 1
        check_applied(p0, g, dec, p, scal, 0.0)
    if kind == "linear":
        assert float(want) == 0.0                            # past the end the rate is 0 ...
        assert torch.equal(bits(p), bits(p0))                # ... and the step moves nothing


def guard_of(counters, log_f, log_i, loss, skip=1):
    rows = 0 if log_f is None else log_f.shape[0]
    return _lib.StepGuardC(counters.data_ptr(), None if log_f is None else log_f.data_ptr(), None if log_i is None else log_i.data_ptr(), rows,
                           None if loss is None else loss.data_ptr(), skip)


def bad_gradient(g, kind):
    g = g.clone()
    if kind == "inf":
        g[len(g) // 2] = float("inf")
    elif kind == "nan":
        g[len(g) - 1] = float("nan")
    else:
        g.fill_(1e19)                                        # finite; every square 1e38, a partial's sum past fp32
    return g


@pytest.mark.parametrize("kind", ["inf", "nan", "overflow"])
def test_guarded_skips_nonfinite_gradients_and_a_good_step_resets_in_a_row(kind):
    n, R = 4099, 4
    p, g, dec, step, scal, part = make(n)
    step.fill_(7)
    counters = torch.zeros(4, dtype=torch.int64, device="cuda")
    log_f, log_i = nans((R, _lib.STEP_LOG_FLOATS)), torch.full((R, 2), -1, dtype=torch.int64, device="cuda")
    loss = torch.tensor([0.625], device="cuda")
    gd = guard_of(counters, log_f, log_i, loss)
    bad = bad_gradient(g, kind)
    assert kind != "overflow" or bool(torch.isfinite(bad).all())
    p0 = p.clone()
    for attempt in (0, 1):
        scal.fill_(float("nan"))
        _lib.check(sgd(p, bad, dec, n, 1.0, step, scal, part, guard=gd))
        torch.cuda.synchronize()
        sc = scal.cpu()
        assert torch.equal(bits(p), bits(p0)) and int(step[0]) == 7
        assert float(sc[5]) == 1.0 and float(sc[0]) == 0.0 and not math.isfinite(float(sc[3])) and float(sc[4]) == LR
        assert math.isnan(float(sc[1])) and math.isnan(float(sc[2]))                         # left unwritten
        assert counters.tolist() == [attempt + 1, attempt + 1, attempt + 1, 0]
        row = log_f[attempt].cpu()
        assert float(row[0]) == 0.625 and not math.isfinite(float(row[1])) and float(row[2]) == 0.0 and float(row[3]) == LR
        assert float(row[4]) == _lib.STEP_LOG_SKIPPED and log_i[attempt].tolist() == [attempt, 7]
    _lib.check(sgd(p, g, dec, n, 1.0, step, scal, part, guard=gd))
    torch.cuda.synchronize()
    check_applied(p0, g, dec, p, scal, 1.0)
    assert float(scal[5]) == 0.0 and int(step[0]) == 8 and counters.tolist() == [3, 2, 0, 0]
    assert float(log_f[2, 4]) == _lib.STEP_LOG_APPLIED and log_i[2].tolist() == [2, 8]


def test_guard_that_does_not_skip_applies_the_step_and_logs_flag_2():
    n = 1025
    p, g, dec, step, scal, part = make(n)
    counters = torch.zeros(4, dtype=torch.int64, device="cuda")
    log_f, log_i = nans((2, _lib.STEP_LOG_FLOATS)), torch.full((2, 2), -1, dtype=torch.int64, device="cuda")
    bad = bad_gradient(g, "inf")
    p0 = p.clone()
    _lib.check(sgd(p, bad, dec, n, 0.0, step, scal, part, guard=guard_of(counters, log_f, log_i, None, skip=0)))
    torch.cuda.synchronize()
    assert float(scal[5]) == 0.0 and int(step[0]) == 1 and counters.tolist() == [1, 0, 0, 0]
    assert float(log_f[0, 4]) == _lib.STEP_LOG_APPLIED_NONFINITE and math.isnan(float(log_f[0, 0])) and log_i[0].tolist() == [0, 1]
    want = sgd_step_host(p0.cpu().numpy(), bad.cpu().numpy(), dec.cpu().numpy(), scal[0].cpu().numpy(), scal[4].cpu().numpy(), np.float32(WD))
    assert np.array_equal(p.cpu().numpy().view(np.int32), want.view(np.int32))      # (the Inf element became -Inf; the others moved as ever)
    assert not bool(torch.isfinite(p).all())


def test_refusals_return_minus_2_and_launch_nothing():
    n = 1025
    p, g, dec, step, scal, part = make(n)
    counters = torch.zeros(4, dtype=torch.int64, device="cuda")
    p0 = p.clone()
    ok = dict(p=p, g=g, dec=dec, n=n, max_norm=1.0, step=step, scal=scal, part=part)
    cases = [dict(ok, **{k: None}) for k in ("p", "g", "dec", "step", "scal", "part")]
    cases += [dict(ok, n=-1), dict(ok, lr=float("nan")), dict(ok, lr=float("inf")), dict(ok, wd=float("nan")), dict(ok, max_norm=float("inf"))]
    cases += [dict(ok, sched=_lib.LrScheduleC(9, 0, 10)), dict(ok, sched=_lib.LrScheduleC(2, -1, 10)), dict(ok, sched=_lib.LrScheduleC(2, 0, 0)),
              dict(ok, sched=_lib.LrScheduleC(5, 10, 10)), dict(ok, sched=_lib.LrScheduleC(5, 0, 10), lr=1e-8)]
    cases += [dict(ok, guard=_lib.StepGuardC(None, None, None, 0, None, 1)), dict(ok, guard=_lib.StepGuardC(counters.data_ptr(), None, None, -1, None, 1)),
              dict(ok, guard=_lib.StepGuardC(counters.data_ptr(), None, None, 2, None, 1))]
    for kw in cases:
        assert sgd(**kw) == -2, {k: v for k, v in kw.items() if not isinstance(v, torch.Tensor)}
    torch.cuda.synchronize()
    assert int(step[0]) == 0 and bool(torch.isnan(scal).all()) and bool(torch.isnan(part).all()) and torch.equal(p, p0)
    assert counters.tolist() == [0, 0, 0, 0]
