"""pmgt_op_step_segments: pmgt_op_adamw_segments -- several disjoint flat buffers as ONE optimizer, one norm, one clip, one step counter, a
rate per segment -- with a learning-rate schedule, the step guard and SGD.

  * AdamW with neither schedule nor guard is pmgt_op_adamw_segments bit for bit (p, m, v, step, scal[0..4]; that file's sizes and scales).
  * ONE segment at lr_scale 1 is the single-buffer entry bit for bit: AdamW + cosine + guard = pmgt_op_adamw_guarded, SGD + linear + guard =
    pmgt_op_sgd (also on ranges that start 1, 2 and 3 floats into their allocations), counters and log ring included.
  * Several segments under SGD: the joint norm within 1e-5 relative of fp64 (that file's figure), scal[4] pmgt_op_lr_schedule's bits, every
    segment's p BIT-EQUAL to pair_train.sgd_step_host at lr_t = fp32(scal[4]) * fp32(lr_scale).
  * Several segments under AdamW against an fp64 restatement with the joint norm and lr_t * lr_scale, by that file's measure.
  * The guard: ONE Inf or NaN element in ONE segment skips EVERY segment; the next step is step 1 of a run that never saw it.
  * lr_scale 0; the refusals."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.pair_train import sgd_step_host
from pmgt_amd.schedule import lr_lambda
from tests.test_rowops_gpu import ADAM, P, assert_close, nans, stream, ulp

pytestmark = pytest.mark.gpu

ADAMW, SGD = _lib.OPTIMS.index("adamw"), _lib.OPTIMS.index("sgd")
W, T, ROWS = 2, 10, 4


def bits(t):
    return t.view(torch.int32)


def seg_array(segs):
    """segs: [(p, g, m, v, dec, lr_scale)] of device tensors (m, v None: NULL)"""
    arr = (_lib.AdamSegmentC * max(len(segs), 1))()
    for k, (p, g, m, v, dec, scale) in enumerate(segs):
        arr[k] = _lib.AdamSegmentC(p.data_ptr(), g.data_ptr(), None if m is None else m.data_ptr(), None if v is None else v.data_ptr(),
                                   dec.data_ptr(), p.numel(), scale)
    return arr


def step_call(segs, optim, max_norm, step, scal, part, sched=None, guard=None, lr=None, wd=None, count=None):
    a = ADAM
    arr = segs if isinstance(segs, C.Array) or segs is None else seg_array(segs)
    return _lib.hip().pmgt_op_step_segments(arr, (len(segs) if count is None else count), optim, a["lr"] if lr is None else lr,
                                            a["wd"] if wd is None else wd, a["b1"], a["b2"], a["eps"], max_norm, P(step), P(scal), P(part),
                                            None if sched is None else C.byref(sched), None if guard is None else C.byref(guard), stream())


def old_call(segs, max_norm, step, scal, part):
    a = ADAM
    return _lib.hip().pmgt_op_adamw_segments(seg_array(segs), len(segs), a["lr"], a["wd"], a["b1"], a["b2"], a["eps"], max_norm, P(step), P(scal),
                                             P(part), stream())


def make(n, gen, offset=0):
    """p (a view `offset` floats into its allocation), m, v, the decay mask (a view `offset` bytes into its own)"""
    p = torch.randn(n + offset, device="cuda", generator=gen)[offset:]
    dec = (torch.rand(n + offset, device="cuda", generator=gen) < 0.6).to(torch.uint8)[offset:]
    return p, torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), dec


def grad(n, gen, offset=0, scale=1.0):
    return (torch.randn(n + offset, device="cuda", generator=gen) * scale)[offset:]


def schedule(kind):
    return _lib.LrScheduleC(_lib.LR_SCHEDULE_TYPES.index(kind), W, T)


def scheduled_rate(sched, s, lr=ADAM["lr"]):
    """pmgt_op_lr_schedule's float for `s` completed steps"""
    out = torch.zeros(1, device="cuda")
    _lib.check(_lib.hip().pmgt_op_lr_schedule(C.byref(sched), lr, s, 1, P(out), stream()))
    torch.cuda.synchronize()
    return out.cpu()


class Guard:
    """counters, a ROWS-row ring and a loss scalar on the device"""

    def __init__(self, rows=ROWS, skip=1, loss=0.625):
        self.counters = torch.zeros(4, dtype=torch.int64, device="cuda")
        self.log_f = torch.zeros(max(rows, 1), _lib.STEP_LOG_FLOATS, device="cuda")
        self.log_i = torch.full((max(rows, 1), 2), -1, dtype=torch.int64, device="cuda")
        self.loss = torch.tensor([loss], device="cuda")
        self.c = _lib.StepGuardC(self.counters.data_ptr(), self.log_f.data_ptr() if rows else None, self.log_i.data_ptr() if rows else None, rows,
                                 self.loss.data_ptr(), skip)

    def same(self, other):
        return (torch.equal(self.counters, other.counters) and torch.equal(bits(self.log_f), bits(other.log_f))
                and torch.equal(self.log_i, other.log_i))


@pytest.mark.parametrize("mode", ["off", "inactive", "active"])
@pytest.mark.parametrize("sizes,scales", [((1, 1023), (1.0, 0.1)), ((1025, 7, 4096), (0.1, 1.0, 2.5)), ((1 << 20, 3), (0.25, 1.0))],
                         ids=["1+1023", "1025+7+4096", "2^20+3"])
def test_adamw_without_options_is_pmgt_op_adamw_segments_bit_for_bit(sizes, scales, mode):
    gen = torch.Generator(device="cuda").manual_seed(sum(sizes))
    mine = [make(n, gen) for n in sizes]
    theirs = [(p.clone(), m.clone(), v.clone(), dec) for p, m, v, dec in mine]
    step, step2 = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    scal, scal2, part, part2 = nans((8,)), nans((8,)), nans((1024 * len(sizes),)), nans((1024 * len(sizes),))
    for t in (1, 2, 3):
        gs = [grad(n, gen, scale=0.5 * t) for n in sizes]
        norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs))
        max_norm = {"off": 0.0, "inactive": 10.0 * norm + 1.0, "active": 0.01 * norm}[mode]
        _lib.check(step_call([(p, g, m, v, dec, s) for (p, m, v, dec), g, s in zip(mine, gs, scales)], ADAMW, max_norm, step, scal, part))
        _lib.check(old_call([(p, g, m, v, dec, s) for (p, m, v, dec), g, s in zip(theirs, gs, scales)], max_norm, step2, scal2, part2))
        torch.cuda.synchronize()
        assert int(step[0]) == t == int(step2[0])
        assert torch.equal(bits(scal[:5]), bits(scal2[:5])) and bool(torch.isnan(scal[5:]).all())      # unguarded: [5..7] untouched
        assert (float(scal[0]) < 0.02) == (mode == "active")
        for k, (a, b) in enumerate(zip(mine, theirs)):
            for x, y, what in zip(a[:3], b[:3], "pmv"):
                assert torch.equal(bits(x), bits(y)), (what, k, t)


@pytest.mark.parametrize("n", [1, 5, 4095, (1 << 20) + 3])
def test_one_segment_adamw_cosine_guarded_is_pmgt_op_adamw_guarded_bit_for_bit(n):
    a = ADAM
    gen = torch.Generator(device="cuda").manual_seed(n)
    p, m, v, dec = make(n, gen)
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    step, step2 = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    scal, scal2, part, part2 = nans((8,)), nans((8,)), nans((1024,)), nans((1024,))
    sched, gd, gd2 = schedule("cosine"), Guard(), Guard()
    for t in (1, 2, 3):
        g = grad(n, gen, scale=0.5 * t)
        max_norm = 0.5 * float(g.double().norm())
        _lib.check(step_call([(p, g, m, v, dec, 1.0)], ADAMW, max_norm, step, scal, part, sched=sched, guard=gd.c))
        _lib.check(_lib.hip().pmgt_op_adamw_guarded(P(p2), P(g), P(m2), P(v2), P(dec), n, a["lr"], a["wd"], a["b1"], a["b2"], a["eps"], max_norm,
                                                    P(step2), P(scal2), P(part2), C.byref(sched), C.byref(gd2.c), stream()))
        torch.cuda.synchronize()
        assert int(step[0]) == t == int(step2[0]) and torch.equal(bits(scal[:6]), bits(scal2[:6])) and gd.same(gd2)
        for x, y, what in ((p, p2, "p"), (m, m2, "m"), (v, v2, "v")):
            assert torch.equal(bits(x), bits(y)), (what, t)
    assert gd.counters.tolist() == [3, 0, 0, 0] and gd.log_i[:3].tolist() == [[0, 1], [1, 2], [2, 3]]
    assert float(gd.log_f[0, 3]) == 0.0 and float(gd.log_f[2, 3]) == a["lr"]      # warm-up: 0, lr / 2, lr


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
@pytest.mark.parametrize("n", [1, 5, 4095, (1 << 20) + 3])
def test_one_segment_sgd_linear_guarded_is_pmgt_op_sgd_bit_for_bit(n, offset):
    a = ADAM
    gen = torch.Generator(device="cuda").manual_seed(n + offset)
    p, _, _, dec = make(n, gen, offset)
    assert p.data_ptr() % 16 == 4 * offset and dec.data_ptr() % 4 == offset
    p2 = p.clone() if offset == 0 else torch.cat([p.new_zeros(offset), p])[offset:]      # (the twin at the same alignment)
    step, step2 = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    scal, scal2, part, part2 = nans((8,)), nans((8,)), nans((1024,)), nans((1024,))
    sched, gd, gd2 = schedule("linear"), Guard(), Guard()
    for t in (1, 2, 3):
        g = grad(n, gen, offset, 0.5 * t)
        max_norm = 0.5 * float(g.double().norm())
        _lib.check(step_call([(p, g, None, None, dec, 1.0)], SGD, max_norm, step, scal, part, sched=sched, guard=gd.c))
        _lib.check(_lib.hip().pmgt_op_sgd(P(p2), P(g), P(dec), n, a["lr"], a["wd"], max_norm, P(step2), P(scal2), P(part2), C.byref(sched),
                                          C.byref(gd2.c), stream()))
        torch.cuda.synchronize()
        assert int(step[0]) == t == int(step2[0]) and torch.equal(bits(scal[:6]), bits(scal2[:6])) and gd.same(gd2)
        assert torch.equal(bits(p), bits(p2)), t
    assert gd.counters.tolist() == [3, 0, 0, 0]


SIZES, SCALES, OFFSETS = (1, 1023, 4099), (1.0, 0.1, 2.5), (0, 1, 0)      # (the 1023 floats start one float into their allocation)


def test_several_segments_sgd_linear_is_the_host_restatement_bit_for_bit():
    a = ADAM
    gen = torch.Generator(device="cuda").manual_seed(11)
    state = [make(n, gen, off) for n, off in zip(SIZES, OFFSETS)]
    assert state[1][0].data_ptr() % 16 == 4
    step, scal, part, sched = torch.zeros(1, dtype=torch.int64, device="cuda"), nans((8,)), nans((1024 * 3,)), schedule("linear")
    for t in (1, 2, 3):
        gs = [grad(n, gen, off, 0.5 * t) for n, off in zip(SIZES, OFFSETS)]
        norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs))
        max_norm = 0.5 * norm
        before = [p.clone() for p, _, _, _ in state]
        _lib.check(step_call([(p, g, None, None, dec, s) for (p, _, _, dec), g, s in zip(state, gs, SCALES)], SGD, max_norm, step, scal, part,
                             sched=sched))
        torch.cuda.synchronize()
        sc = scal.cpu()
        assert int(step[0]) == t
        assert abs(float(sc[3]) - norm) <= 1e-5 * norm and abs(float(sc[0]) - 0.5) <= 1e-5 * 0.5
        assert torch.equal(bits(sc[4:5]), bits(scheduled_rate(sched, t - 1))) and float(sc[1]) == float(sc[4]) and float(sc[2]) == 1.0
        for k, ((p, _, _, dec), g, s, p0) in enumerate(zip(state, gs, SCALES, before)):
            want = sgd_step_host(p0.cpu().numpy(), g.cpu().numpy(), dec.cpu().numpy(), clip=sc[0].numpy(),
                                 lr_t=np.float32(sc[4].numpy()) * np.float32(s), wd=np.float32(a["wd"]))
            assert np.array_equal(p.cpu().numpy().view(np.int32), want.view(np.int32)), (k, t)
        assert t == 1 or not torch.equal(state[2][0], before[2])       # (step 1 runs at the warm-up's rate 0)


def test_several_segments_adamw_cosine_against_fp64_with_the_joint_norm():
    a = ADAM
    gen = torch.Generator(device="cuda").manual_seed(12)
    state = [make(n, gen, off) for n, off in zip(SIZES, OFFSETS)]
    step, scal, part, sched = torch.zeros(1, dtype=torch.int64, device="cuda"), nans((8,)), nans((1024 * 3,)), schedule("cosine")
    lam = lr_lambda("cosine", W, T, a["lr"])
    for t in (1, 2, 3):
        gs = [grad(n, gen, off, 0.5 * t) for n, off in zip(SIZES, OFFSETS)]
        norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs))
        max_norm = 0.5 * norm
        before = [(p.clone(), m.clone(), v.clone()) for p, m, v, _ in state]
        _lib.check(step_call([(p, g, m, v, dec, s) for (p, m, v, dec), g, s in zip(state, gs, SCALES)], ADAMW, max_norm, step, scal, part,
                             sched=sched))
        torch.cuda.synchronize()
        sc = scal.cpu().double()
        lr_t, bc1, bc2 = a["lr"] * lam(t - 1), 1 - a["b1"] ** t, 1 - a["b2"] ** t
        assert int(step[0]) == t and abs(float(sc[3]) - norm) <= 1e-5 * norm and abs(float(sc[0]) - 0.5) <= 1e-5 * 0.5
        assert abs(float(sc[4]) - lr_t) <= 1e-6 * lr_t and abs(float(sc[1]) - lr_t / bc1) <= 1e-6 * lr_t / bc1
        assert torch.equal(bits(scal[4:5].cpu()), bits(scheduled_rate(sched, t - 1)))
        for k, ((p, m, v, dec), g, s, (p0, m0, v0)) in enumerate(zip(state, gs, SCALES, before)):
            gg = g.double() * float(sc[0])
            m_ref = a["b1"] * m0.double() + (1 - a["b1"]) * gg
            v_ref = a["b2"] * v0.double() + (1 - a["b2"]) * gg * gg
            lr = lr_t * s
            p_ref = p0.double() * (1 - lr * a["wd"] * dec.double()) - (lr / bc1) * m_ref / (v_ref.sqrt() / math.sqrt(bc2) + a["eps"])
            assert_close(m, m_ref, torch.float32, ulps=16, floor=1e-7, what=f"m of segment {k} (step {t})")
            assert_close(v, v_ref, torch.float32, ulps=16, floor=1e-7, what=f"v of segment {k} (step {t})")
            err = (p.double() - p_ref).abs()
            bound = 2 * ulp(p_ref, torch.float32) + 1e-3 * lr_t * s
            assert bool((err <= bound).all()), f"p of segment {k} (step {t}): max error {float(err.max())!r}"


@pytest.mark.parametrize("optim", [ADAMW, SGD], ids=["adamw", "sgd"])
@pytest.mark.parametrize("value", [math.inf, math.nan], ids=["inf", "nan"])
def test_one_bad_element_in_one_segment_skips_every_segment(value, optim):
    a = ADAM
    gen = torch.Generator(device="cuda").manual_seed(13)
    state = [make(n, gen, off) for n, off in zip(SIZES, OFFSETS)]
    twin = [(p.clone(), m.clone(), v.clone(), dec) for p, m, v, dec in state]
    gs = [grad(n, gen, off) for n, off in zip(SIZES, OFFSETS)]
    bad = [g.clone() for g in gs]
    bad[2][2048] = value
    segs = lambda st, grads: [(p, g, m, v, dec, s) for (p, m, v, dec), g, s in zip(st, grads, SCALES)]
    step, scal, part, sched, gd = torch.zeros(1, dtype=torch.int64, device="cuda"), nans((8,)), nans((1024 * 3,)), schedule("cosine"), Guard()
    step.fill_(1)                                            # one applied step so far: the rate is lambda(1) lr = lr / 2
    keep = [tuple(x.clone() for x in s[:3]) for s in state]
    _lib.check(step_call(segs(state, bad), optim, 1.0, step, scal, part, sched=sched, guard=gd.c))
    torch.cuda.synchronize()
    sc = scal.cpu()
    for s, k in zip(state, keep):
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(s[:3], k))
    assert int(step[0]) == 1 and float(sc[5]) == 1.0 and float(sc[0]) == 0.0 and not math.isfinite(float(sc[3]))
    rate = scheduled_rate(sched, 1)
    assert torch.equal(bits(sc[4:5]), bits(rate)) and float(rate) == a["lr"] / 2 and gd.counters.tolist() == [1, 1, 1, 0]
    row = gd.log_f[0].cpu()
    assert float(row[0]) == 0.625 and not math.isfinite(float(row[1])) and float(row[2]) == 0.0 and float(row[3]) == float(rate)
    assert float(row[4]) == _lib.STEP_LOG_SKIPPED and gd.log_i[0].tolist() == [0, 1]
    # the next, finite step applies, and is the step of a run that never saw the bad batch: the schedule and the bias corrections count applied steps
    step2, scal2, part2, gd2 = torch.ones(1, dtype=torch.int64, device="cuda"), nans((8,)), nans((1024 * 3,)), Guard()
    _lib.check(step_call(segs(state, gs), optim, 1.0, step, scal, part, sched=sched, guard=gd.c))
    _lib.check(step_call(segs(twin, gs), optim, 1.0, step2, scal2, part2, sched=sched, guard=gd2.c))
    torch.cuda.synchronize()
    assert int(step[0]) == 2 == int(step2[0]) and torch.equal(bits(scal[:6]), bits(scal2[:6])) and float(scal[5]) == 0.0
    assert gd.counters.tolist() == [2, 1, 0, 0] and gd.log_i[1].tolist() == [1, 2] and float(gd.log_f[1, 4]) == _lib.STEP_LOG_APPLIED
    for s, w, k in zip(state, twin, keep):
        assert all(torch.equal(bits(x), bits(y)) for x, y in zip(s[:3], w[:3])) and not torch.equal(s[0], k[0])
    # skip_nonfinite = 0 with a ring: the row says non-finite but applied
    gd3 = Guard(skip=0)
    _lib.check(step_call(segs(twin, bad), optim, 0.0, step2, scal2, part2, sched=sched, guard=gd3.c))
    torch.cuda.synchronize()
    assert int(step2[0]) == 3 and float(scal2[5]) == 0.0 and gd3.counters.tolist() == [1, 0, 0, 0]
    assert float(gd3.log_f[0, 4]) == _lib.STEP_LOG_APPLIED_NONFINITE and gd3.log_i[0].tolist() == [0, 3]


def test_lr_scale_zero():
    gen = torch.Generator(device="cuda").manual_seed(5)
    (p0, m0, v0, d0), (p1, m1, v1, d1) = make(4099, gen), make(513, gen)
    keep0, keep1 = p0.clone(), p1.clone()
    step, scal, part = torch.zeros(1, dtype=torch.int64, device="cuda"), nans((8,)), nans((2048,))
    for _ in range(2):
        g0, g1 = grad(4099, gen), grad(513, gen)
        _lib.check(step_call([(p0, g0, m0, v0, d0, 0.0), (p1, g1, m1, v1, d1, 1.0)], ADAMW, 1.0, step, scal, part))
    torch.cuda.synchronize()
    assert torch.equal(bits(p0), bits(keep0))                # not even the decay touches it
    assert bool((m0 != 0).all()) and bool((v0 > 0).all()) and not torch.equal(p1, keep1) and int(step[0]) == 2
    keep1 = p1.clone()
    _lib.check(step_call([(p0, g0, None, None, d0, 0.0), (p1, g1, None, None, d1, 1.0)], SGD, 1.0, step, scal, part))
    torch.cuda.synchronize()
    assert torch.equal(bits(p0), bits(keep0)) and not torch.equal(p1, keep1) and int(step[0]) == 3


def test_refusals():
    gen = torch.Generator(device="cuda").manual_seed(7)
    p, m, v, d = make(64, gen)
    g = torch.ones(64, device="cuda")
    keep = p.clone()
    step, scal, part = torch.zeros(1, dtype=torch.int64, device="cuda"), nans((8,)), nans((9 * 1024,))
    counters = torch.zeros(4, dtype=torch.int64, device="cuda")
    ok = (p, g, m, v, d, 1.0)
    null = torch.empty(0, device="cuda")                     # data_ptr() == 0
    assert null.data_ptr() == 0
    call = lambda segs=(ok,), optim=ADAMW, **kw: step_call(list(segs), optim, kw.pop("max_norm", 0.0), kw.pop("step", step), kw.pop("scal", scal),
                                                           kw.pop("part", part), **kw)
    # what pmgt_op_adamw_segments refuses
    rcs = [call([]), call([ok] * 9), call([(p, g, m, v, d, -0.5)]), call([(p, g, m, v, d, float("inf"))]), call([(p, g, m, v, d, float("nan"))]),
           call(step=null), call(scal=null), call(part=null), step_call(None, ADAMW, 0.0, step, scal, part, count=1)]
    for optim in (ADAMW, SGD):
        for field in ("p", "g", "decay") + (("m", "v") if optim == ADAMW else ()):      # a NULL m or v under AdamW
            seg = _lib.AdamSegmentC(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), d.data_ptr(), 64, 1.0)
            setattr(seg, field, None)
            rcs.append(step_call((_lib.AdamSegmentC * 1)(seg), optim, 0.0, step, scal, part, count=1))
    rcs.append(step_call((_lib.AdamSegmentC * 1)(_lib.AdamSegmentC(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), d.data_ptr(), -1, 1.0)),
                         ADAMW, 0.0, step, scal, part, count=1))
    # an optim that is neither value; lr, wd or max_norm not finite
    rcs += [call(optim=2), call(optim=-1), call(lr=float("nan")), call(lr=float("inf")), call(wd=float("nan")), call(max_norm=float("inf")),
            call(max_norm=float("nan"))]
    # what pmgt_op_adamw_guarded refuses of a given schedule or guard
    rcs += [call(sched=_lib.LrScheduleC(9, 0, 10)), call(sched=_lib.LrScheduleC(2, -1, 10)), call(sched=_lib.LrScheduleC(2, 0, 0)),
            call(sched=_lib.LrScheduleC(5, 10, 10)), call(sched=_lib.LrScheduleC(5, 0, 10), lr=1e-8),
            call(guard=_lib.StepGuardC(None, None, None, 0, None, 1)), call(guard=_lib.StepGuardC(counters.data_ptr(), None, None, -1, None, 1)),
            call(guard=_lib.StepGuardC(counters.data_ptr(), None, None, 2, None, 1))]
    assert rcs == [-2] * len(rcs), rcs
    torch.cuda.synchronize()
    assert int(step[0]) == 0 and torch.equal(bits(p), bits(keep)) and bool(torch.isnan(scal).all()) and bool(torch.isnan(part).all())
    assert counters.tolist() == [0, 0, 0, 0]
    eight = [(p[8 * k: 8 * k + 8], g[8 * k: 8 * k + 8], m[8 * k: 8 * k + 8], v[8 * k: 8 * k + 8], d[8 * k: 8 * k + 8], 1.0) for k in range(8)]
    assert _lib.ADAM_MAX_SEGMENTS == 8 and call(eight) == 0 and call(eight, optim=SGD, sched=schedule("linear")) == 0      # the most one call takes
    torch.cuda.synchronize()
    assert int(step[0]) == 2 and abs(float(scal[3]) - 8.0) < 1e-5 and not torch.equal(p, keep)      # norm of 64 ones
