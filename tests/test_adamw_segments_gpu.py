"""pmgt_op_adamw_segments: global-norm clip + AdamW over several disjoint flat buffers as ONE optimizer -- one norm over all segments, one
clip coefficient, one step counter, one pair of bias corrections, per segment a rate of its own (lr_scale multiplies the step size and the
decay rate).

  * ONE segment, lr_scale 1: p, m, v, step and scal[0..3] BIT-EQUAL to pmgt_op_adamw over three steps (the arithmetic is that kernel's).
  * Several segments, three steps, against the fp64 restatement below with the JOINT norm, by the measure of
    tests/test_rowops_gpu.py::test_clip_and_adamw_three_steps (whose helpers are imported): norm and coefficient within 1e-5 relative, m and
    v within 16 ulp with floor 1e-7, p within 2 ulp + 1e-3 lr lr_scale (one step moves p by about lr lr_scale).
  * lr_scale 0 leaves that segment's p untouched bit for bit while its m and v move; a clip that is active only because of the OTHER
    segment's gradient scales both; the refusals."""
import ctypes as C
import math

import pytest
import torch

from pmgt_amd import _lib
from tests.test_rowops_gpu import ADAM, P, assert_close, nans, stream, ulp

pytestmark = pytest.mark.gpu


def segments_call(segs, max_norm, step, scal, part, lr=None, count=None):
    """segs: [(p, g, m, v, dec, lr_scale)] of device tensors"""
    a = ADAM
    arr = (_lib.AdamSegmentC * max(len(segs), 1))()
    for k, (p, g, m, v, dec, scale) in enumerate(segs):
        arr[k] = _lib.AdamSegmentC(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), dec.data_ptr(), p.numel(), scale)
    return _lib.hip().pmgt_op_adamw_segments(arr, len(segs) if count is None else count, a["lr"] if lr is None else lr, a["wd"], a["b1"], a["b2"],
                                             a["eps"], max_norm, P(step), P(scal), P(part), stream())


def make(n, gen):
    p = torch.randn(n, device="cuda", generator=gen)
    dec = (torch.rand(n, device="cuda", generator=gen) < 0.6).to(torch.uint8)
    return p, torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda"), dec


@pytest.mark.parametrize("mode", ["off", "inactive", "active"])
@pytest.mark.parametrize("n", [1, 5, 4095, (1 << 20) + 3])
def test_one_segment_is_pmgt_op_adamw_bit_for_bit(n, mode):
    a = ADAM
    gen = torch.Generator(device="cuda").manual_seed(n)
    p, m, v, dec = make(n, gen)
    p2, m2, v2 = p.clone(), m.clone(), v.clone()
    step, step2 = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    scal, scal2, part, part2 = nans((4,)), nans((8,)), nans((1024,)), nans((1024,))
    for t in (1, 2, 3):
        g = torch.randn(n, device="cuda", generator=gen) * (0.5 * t)
        norm = float(g.double().norm())
        max_norm = {"off": 0.0, "inactive": 10.0 * norm + 1.0, "active": 0.01 * norm}[mode]
        _lib.check(_lib.hip().pmgt_op_adamw(P(p), P(g), P(m), P(v), P(dec), n, a["lr"], a["wd"], a["b1"], a["b2"], a["eps"], max_norm, P(step),
                                            P(scal), P(part), stream()))
        _lib.check(segments_call([(p2, g, m2, v2, dec, 1.0)], max_norm, step2, scal2, part2))
        torch.cuda.synchronize()
        assert int(step2[0]) == t == int(step[0])
        assert torch.equal(scal.view(torch.int32), scal2[:4].view(torch.int32))
        assert (float(scal2[0]) < 0.02) == (mode == "active")
        for x, y, what in ((p, p2, "p"), (m, m2, "m"), (v, v2, "v")):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), (what, t)


def reference_step(segs, g64, scales, coef, t):
    """fp64 restatement of one step over every segment, with the kernel's clip coefficient (itself checked against the fp64 one): clip_grad_norm
    over the JOINT norm, then adamw_step per segment at lr * lr_scale -> [(p_ref, m_ref, v_ref)]"""
    a = ADAM
    bc1, bc2 = 1 - a["b1"] ** t, 1 - a["b2"] ** t
    out = []
    for (p, _, m, v, dec, _), g, s in zip(segs, g64, scales):
        gg = g * coef
        m_ref = a["b1"] * m.double() + (1 - a["b1"]) * gg
        v_ref = a["b2"] * v.double() + (1 - a["b2"]) * gg * gg
        lr = a["lr"] * s
        p_ref = p.double() * (1 - lr * a["wd"] * dec.double()) - (lr / bc1) * m_ref / (v_ref.sqrt() / math.sqrt(bc2) + a["eps"])
        out.append((p_ref, m_ref, v_ref))
    return out


@pytest.mark.parametrize("mode", ["off", "inactive", "active"])
@pytest.mark.parametrize("sizes,scales", [((1, 1023), (1.0, 0.1)), ((1025, 7, 4096), (0.1, 1.0, 2.5)), ((1 << 20, 3), (0.25, 1.0))],
                         ids=["1+1023", "1025+7+4096", "2^20+3"])
def test_segments_three_steps_against_fp64_with_the_joint_norm(sizes, scales, mode):
    a = ADAM
    gen = torch.Generator(device="cuda").manual_seed(sum(sizes))
    state = [make(n, gen) for n in sizes]
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    scal, part = nans((8,)), nans((1024 * len(sizes),))
    for t in (1, 2, 3):
        gs = [torch.randn(n, device="cuda", generator=gen) * (0.5 * t) for n in sizes]
        norm = math.sqrt(sum(float((g.double() ** 2).sum()) for g in gs))
        max_norm = {"off": 0.0, "inactive": 10.0 * norm + 1.0, "active": 0.01 * norm}[mode]
        segs = [(p, g, m, v, dec, s) for (p, m, v, dec), g, s in zip(state, gs, scales)]
        before = [(p.clone(), None, m.clone(), v.clone(), dec, s) for p, _, m, v, dec, s in segs]
        _lib.check(segments_call(segs, max_norm, step, scal, part))
        torch.cuda.synchronize()
        assert int(step[0]) == t                             # ONE increment per call, however many segments
        coef = min(max_norm / (norm + 1e-6), 1.0) if max_norm > 0 else 1.0
        bc1, bc2 = 1 - a["b1"] ** t, 1 - a["b2"] ** t
        sc = scal.cpu().double()
        assert abs(float(sc[3]) - norm) <= 1e-5 * norm and abs(float(sc[0]) - coef) <= 1e-5 * coef
        assert (float(sc[0]) < 0.02) if mode == "active" else float(sc[0]) == 1.0
        assert abs(float(sc[1]) - a["lr"] / bc1) <= 1e-6 * a["lr"] / bc1 and abs(float(sc[2]) - 1 / math.sqrt(bc2)) <= 1e-6 / math.sqrt(bc2)
        refs = reference_step(before, [g.double() for g in gs], scales, float(sc[0]), t)
        for k, ((p, _, m, v, _, s), (p_ref, m_ref, v_ref)) in enumerate(zip(segs, refs)):
            assert_close(m, m_ref, torch.float32, ulps=16, floor=1e-7, what=f"m of segment {k} (step {t})")
            assert_close(v, v_ref, torch.float32, ulps=16, floor=1e-7, what=f"v of segment {k} (step {t})")
            err = (p.double() - p_ref).abs()
            bound = 2 * ulp(p_ref, torch.float32) + 1e-3 * a["lr"] * s
            assert bool((err <= bound).all()), f"p of segment {k} (step {t}): max error {float(err.max())!r}"


def test_lr_scale_zero_freezes_p_and_moves_the_moments():
    gen = torch.Generator(device="cuda").manual_seed(5)
    (p0, m0, v0, d0), (p1, m1, v1, d1) = make(4099, gen), make(513, gen)
    keep0, keep1 = p0.clone(), p1.clone()
    step, scal, part = torch.zeros(1, dtype=torch.int64, device="cuda"), nans((8,)), nans((2048,))
    for _ in range(2):
        g0, g1 = torch.randn(4099, device="cuda", generator=gen), torch.randn(513, device="cuda", generator=gen)
        _lib.check(segments_call([(p0, g0, m0, v0, d0, 0.0), (p1, g1, m1, v1, d1, 1.0)], 1.0, step, scal, part))
    torch.cuda.synchronize()
    assert torch.equal(p0.view(torch.int32), keep0.view(torch.int32))      # not even the decay touches it
    assert bool((m0 != 0).all()) and bool((v0 > 0).all()) and not torch.equal(p1, keep1) and int(step[0]) == 2


def test_a_clip_caused_by_the_other_segment_scales_both():
    """segment 0 alone has norm 0.5 < max_norm = 1; with segment 1's gradient the joint norm is about 100: both first moments are
    (1 - b1) coef g with the ONE coefficient"""
    a = ADAM
    n0, n1 = 2500, 10000
    g0, g1 = torch.full((n0,), 0.01, device="cuda"), torch.ones(n1, device="cuda")      # norms 0.5 and 100
    gen = torch.Generator(device="cuda").manual_seed(6)
    (p0, m0, v0, d0), (p1, m1, v1, d1) = make(n0, gen), make(n1, gen)
    step, scal, part = torch.zeros(1, dtype=torch.int64, device="cuda"), nans((8,)), nans((2048,))
    _lib.check(segments_call([(p0, g0, m0, v0, d0, 1.0), (p1, g1, m1, v1, d1, 1.0)], 1.0, step, scal, part))
    torch.cuda.synchronize()
    norm = math.sqrt(0.25 + 10000.0)
    coef = 1.0 / (norm + 1e-6)
    assert abs(float(scal[3]) - norm) <= 1e-5 * norm and abs(float(scal[0]) - coef) <= 1e-5 * coef
    for m, g in ((m0, 0.01), (m1, 1.0)):
        want = (1 - a["b1"]) * g * float(scal[0])
        assert bool(((m.double() - want).abs() <= 4e-7 * want).all())
    # alone, segment 0 is not clipped
    m0.zero_(), v0.zero_()
    _lib.check(segments_call([(p0, g0, m0, v0, d0, 1.0)], 1.0, step, scal, part))
    torch.cuda.synchronize()
    assert float(scal[0]) == 1.0


def test_refusals():
    gen = torch.Generator(device="cuda").manual_seed(7)
    p, m, v, d = make(64, gen)
    g = torch.ones(64, device="cuda")
    keep = p.clone()
    step, scal, part = torch.zeros(1, dtype=torch.int64, device="cuda"), nans((8,)), nans((9 * 1024,))
    ok = (p, g, m, v, d, 1.0)
    null = torch.empty(0, device="cuda")                     # data_ptr() == 0
    assert null.data_ptr() == 0
    rcs = [segments_call([], 0.0, step, scal, part), segments_call([ok] * 9, 0.0, step, scal, part),
           segments_call([(p, g, m, v, d, -0.5)], 0.0, step, scal, part), segments_call([(p, g, m, v, d, float("inf"))], 0.0, step, scal, part),
           segments_call([(p, g, m, v, d, float("nan"))], 0.0, step, scal, part),
           segments_call([ok], 0.0, null, scal, part), segments_call([ok], 0.0, step, null, part), segments_call([ok], 0.0, step, scal, null)]
    arr = (_lib.AdamSegmentC * 1)(_lib.AdamSegmentC(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), d.data_ptr(), -1, 1.0))
    a = ADAM
    call = lambda s: _lib.hip().pmgt_op_adamw_segments(s, 1, a["lr"], a["wd"], a["b1"], a["b2"], a["eps"], 0.0, P(step), P(scal), P(part), stream())
    rcs.append(call(arr))
    for field in ("p", "g", "m", "v", "decay"):
        seg = _lib.AdamSegmentC(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), d.data_ptr(), 64, 1.0)
        setattr(seg, field, None)
        rcs.append(call((_lib.AdamSegmentC * 1)(seg)))
    rcs.append(_lib.hip().pmgt_op_adamw_segments(None, 1, a["lr"], a["wd"], a["b1"], a["b2"], a["eps"], 0.0, P(step), P(scal), P(part), stream()))
    assert rcs == [-2] * len(rcs)
    torch.cuda.synchronize()
    assert int(step[0]) == 0 and torch.equal(p, keep) and torch.isnan(scal).all()
    eight = [(p[8 * k: 8 * k + 8], g[8 * k: 8 * k + 8], m[8 * k: 8 * k + 8], v[8 * k: 8 * k + 8], d[8 * k: 8 * k + 8], 1.0) for k in range(8)]
    assert _lib.ADAM_MAX_SEGMENTS == 8 and segments_call(eight, 0.0, step, scal, part) == 0      # the most segments one call takes
    torch.cuda.synchronize()
    assert int(step[0]) == 1 and abs(float(scal[3]) - 8.0) < 1e-5 and not torch.equal(p, keep)      # norm of 64 ones
