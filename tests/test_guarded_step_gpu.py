"""The guarded optimizer step (pmgt_amd/ops/optimizer_step.hip: the guarded instantiation of adam_prepare_step_kernel / adamw_step_kernel)
from the single-kernel entry up to captured steps, checkpoints and fit: a step whose global gradient norm is not finite is skipped on the
device, every step is counted, and a device ring keeps one row per step.

Bounds.  Everything here is bit-exact (torch.equal, ==): an applied guarded step is the unguarded step's arithmetic in the same order, a
skipped one writes no parameter byte, and the log copies fp32 values the step computed anyway.  An Inf or NaN float is ordinary data to
these kernels: nothing here provokes a fault."""
import copy
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from tests import golden_util as gu
from tests.test_engine_gpu import dev_batch, make_engine
from tests.test_lr_schedule_gpu import _sched
from tests.test_resume_gpu import fit_world, fresh_engine, live_inputs
from tests.test_rowops_gpu import ADAM, H, P, check, nans, stream

pytestmark = pytest.mark.gpu

N = 4099                 # 5 norm partials (1024 elements per block) and a 3-element tail in the 4-wide AdamW loop
NO_DROP = dict(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)


@pytest.fixture(autouse=True)
def _no_graph_left_behind():
    """Captured steps are destroyed here, with the GPU idle (see tests/test_lr_schedule_gpu.py)."""
    yield
    import gc
    torch.cuda.synchronize()
    gc.collect()


def bits(t):
    return t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


# =========================================================================================== the single-kernel entry
class OpState:
    """p, g-independent optimizer state of one op run over n elements, with the guard's buffers."""

    def __init__(self, p, m, v, step=0, rows=4, n=N):
        self.p, self.m, self.v, self.n = p.clone(), m.clone(), v.clone(), n
        self.step = torch.full((1,), step, dtype=torch.int64, device="cuda")
        self.scal, self.part = nans((8,)), nans((1024,))
        self.counters = torch.zeros(4, dtype=torch.int64, device="cuda")
        self.rows = rows
        self.log_f = nans((rows, 8))
        self.log_i = torch.full((rows, 2), -1, dtype=torch.int64, device="cuda")

    def unguarded(self, g, dec, max_norm, sc):
        a = ADAM
        if sc is None:
            check(H().pmgt_op_adamw(P(self.p), P(g), P(self.m), P(self.v), P(dec), self.n, a["lr"], a["wd"], a["b1"], a["b2"], a["eps"], max_norm,
                                    P(self.step), P(self.scal), P(self.part), stream()))
        else:
            check(H().pmgt_op_adamw_scheduled(P(self.p), P(g), P(self.m), P(self.v), P(dec), self.n, a["lr"], a["wd"], a["b1"], a["b2"], a["eps"],
                                              max_norm, P(self.step), P(self.scal), P(self.part), C.byref(sc), stream()))

    def guarded(self, g, dec, max_norm, sc, skip, loss=None):
        from pmgt_amd import _lib
        a = ADAM
        gd = _lib.StepGuardC(P(self.counters), P(self.log_f), P(self.log_i), self.rows, None if loss is None else P(loss), skip)
        check(H().pmgt_op_adamw_guarded(P(self.p), P(g), P(self.m), P(self.v), P(dec), self.n, a["lr"], a["wd"], a["b1"], a["b2"], a["eps"], max_norm,
                                        P(self.step), P(self.scal), P(self.part), None if sc is None else C.byref(sc), C.byref(gd), stream()))

    def tensors(self):
        return self.p, self.m, self.v, self.step


def op_inputs(seed, n=N):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    p = torch.randn(n, device="cuda", generator=gen)
    m = torch.randn(n, device="cuda", generator=gen) * 0.1
    v = torch.rand(n, device="cuda", generator=gen) * 0.01
    dec = (torch.rand(n, device="cuda", generator=gen) < 0.6).to(torch.uint8)
    gs = [torch.randn(n, device="cuda", generator=gen) * (0.5 * t) for t in (1, 2, 3)]
    return p, m, v, dec, gs


@pytest.mark.parametrize("skip", [0, 1])
@pytest.mark.parametrize("sched", [None, ("linear", 2, 10)])
@pytest.mark.parametrize("max_norm", [0.0, 1.0])
def test_good_steps_are_bit_identical_to_the_unguarded_entries(max_norm, sched, skip):
    """Three consecutive steps from random p, g, m, v: p, m, v, step and scal[0..4] ([0..3] against pmgt_op_adamw, whose scal is [4])
    equal pmgt_op_adamw / pmgt_op_adamw_scheduled bit for bit, guarding on or off; scal[5] = 0, the counters count, the log holds the
    rows."""
    p, m, v, dec, gs = op_inputs(11)
    sc = None if sched is None else _sched(*sched)
    a, b = OpState(p, m, v, step=3), OpState(p, m, v, step=3)
    loss = torch.tensor([0.75], device="cuda")
    k = 4 if sc is None else 5
    for t, g in enumerate(gs):
        a.unguarded(g, dec, max_norm, sc)
        b.guarded(g, dec, max_norm, sc, skip, loss)
        torch.cuda.synchronize()
        for x, y in zip(a.tensors(), b.tensors()):
            assert torch.equal(x, y)
        assert same_bits(a.scal[:k], b.scal[:k]), (a.scal, b.scal)
        assert float(b.scal[5]) == 0.0 and bool(torch.isnan(b.scal[6:]).all())
        if sc is None:
            assert float(b.scal[4]) == ADAM["lr"]
        assert b.counters.tolist() == [t + 1, 0, 0, 0]
        row = b.log_f[t].tolist()
        assert row[0] == 0.75 and row[1:5] == [float(b.scal[3]), float(b.scal[0]), float(b.scal[4]), 0.0]
        assert b.log_i[t].tolist() == [t, 3 + t + 1]
    assert int(b.step[0]) == 6 and bool(torch.isfinite(b.p).all()) and not torch.equal(b.p, p)


@pytest.mark.parametrize("max_norm", [0.0, 1.0])
@pytest.mark.parametrize("n", [1, 3, 4, 1024, 1025, 4099])
def test_every_entry_runs_one_step_body_at_the_edge_sizes(n, max_norm):
    """pmgt_op_adamw, pmgt_op_adamw_scheduled with the constant schedule and pmgt_op_adamw_guarded with a NULL schedule (guarding off and
    on) leave p, m, v, step and scal[0..3] bit-identical over two consecutive steps from random p, g, m, v.  n: a single lane, a tail-only
    group of the 4-wide AdamW loop, exactly one group, exactly one norm partial (1024 elements), a second partial with a one-element
    tail, and N.  The scheduled entry leaves scal[5..7] alone (still NaN), the guarded one writes scal[5] = 0 and leaves [6..7]."""
    p, m, v, dec, gs = op_inputs(14, n)
    const = _sched("constant", 0, 0)
    plain, scheduled, counting, skipping = (OpState(p, m, v, n=n) for _ in range(4))
    for t, g in enumerate(gs[:2]):
        plain.unguarded(g, dec, max_norm, None)
        scheduled.unguarded(g, dec, max_norm, const)
        counting.guarded(g, dec, max_norm, None, 0)
        skipping.guarded(g, dec, max_norm, None, 1)
        torch.cuda.synchronize()
        assert int(plain.step[0]) == t + 1 and bool(torch.isfinite(plain.scal[:4]).all()) and not same_bits(plain.p, p)
        for other in (scheduled, counting, skipping):
            for x, y in zip(plain.tensors(), other.tensors()):
                assert same_bits(x, y)
            assert same_bits(plain.scal[:4], other.scal[:4]), (plain.scal, other.scal)
        assert bool(torch.isnan(scheduled.scal[5:]).all())
        for guarded in (counting, skipping):
            assert float(guarded.scal[5]) == 0.0 and bool(torch.isnan(guarded.scal[6:]).all())


def poison(g, how):
    """-> (poisoned copy, restored copy).  "overflow": two finite elements of 1.5e19 in ONE lane's 4-wide load, so the fp32 partial of
    their squares (2 x 2.25e38 > 3.4e38) overflows although no element and no single square does; the restored gradient has ones there."""
    bad = g.clone()
    if how == "+inf":
        bad[0] = math.inf
    elif how == "-inf":
        bad[N - 1] = -math.inf
    elif how == "nan":
        bad[2048] = math.nan
    else:
        g = g.clone()
        g[100:102] = 1.0
        bad[100:102] = 1.5e19
    return bad, g


@pytest.mark.parametrize("how", ["+inf", "-inf", "nan", "overflow"])
def test_a_bad_step_is_skipped_and_the_next_one_is_the_unguarded_step(how):
    p, m, v, dec, gs = op_inputs(12)
    bad, good = poison(gs[0], how)
    sc = _sched("linear", 2, 10)
    a, b = OpState(p, m, v, step=3), OpState(p, m, v, step=3)
    b.guarded(bad, dec, 1.0, sc, 1)
    torch.cuda.synchronize()
    assert same_bits(b.p, p) and same_bits(b.m, m) and same_bits(b.v, v) and int(b.step[0]) == 3
    assert float(b.scal[5]) == 1.0 and float(b.scal[0]) == 0.0 and not math.isfinite(float(b.scal[3]))
    assert b.counters.tolist() == [1, 1, 1, 0]
    assert b.log_f[0, 4].item() == 1.0 and b.log_i[0].tolist() == [0, 3] and math.isnan(b.log_f[0, 0].item())       # NULL loss pointer: NaN
    # the rate the step would have used: the one the applied step then uses (the skip consumed no schedule position)
    lr_skipped = float(b.scal[4])
    a.unguarded(good, dec, 1.0, sc)
    b.guarded(good, dec, 1.0, sc, 1)
    torch.cuda.synchronize()
    for x, y in zip(a.tensors(), b.tensors()):
        assert torch.equal(x, y)
    assert same_bits(a.scal[:5], b.scal[:5]) and float(b.scal[5]) == 0.0 and float(b.scal[4]) == lr_skipped
    assert b.counters.tolist() == [2, 1, 0, 0]
    assert b.log_f[1, 4].item() == 0.0 and b.log_i[1].tolist() == [1, 4]
    # guarding off: today's behaviour, shown -- the step is applied, counted as an attempt and flagged in the log.  An Inf / NaN element
    # leaves non-finite parameters (inf * coef 0 = NaN; NaN norm -> coef 1); the overflow case has finite elements and an Inf norm, so
    # its clip coefficient is 0 and p stays finite: there the flag and the norm are what shows
    c = OpState(p, m, v, step=3)
    c.guarded(bad, dec, 1.0, sc, 0)
    torch.cuda.synchronize()
    assert int(c.step[0]) == 4 and float(c.scal[5]) == 0.0 and c.counters.tolist() == [1, 0, 0, 0]
    assert c.log_f[0, 4].item() == 2.0 and not math.isfinite(c.log_f[0, 1].item())
    if how != "overflow":
        assert not bool(torch.isfinite(c.p).all())


def test_bad_guards_are_refused():
    from pmgt_amd import _lib
    p, m, v, dec, gs = op_inputs(13)
    s = OpState(p, m, v)
    a = ADAM

    def call(gd):
        return H().pmgt_op_adamw_guarded(P(s.p), P(gs[0]), P(s.m), P(s.v), P(dec), N, a["lr"], a["wd"], a["b1"], a["b2"], a["eps"], 0.0, P(s.step),
                                         P(s.scal), P(s.part), None, None if gd is None else C.byref(gd), stream())
    for gd, word in ((None, "NULL guard"), (_lib.StepGuardC(None, None, None, 0, None, 1), "counters"),
                     (_lib.StepGuardC(P(s.counters), None, None, -1, None, 1), "negative"),
                     (_lib.StepGuardC(P(s.counters), P(s.log_f), None, 4, None, 1), "log pointer"),
                     (_lib.StepGuardC(P(s.counters), None, P(s.log_i), 4, None, 1), "log pointer")):
        assert call(gd) == -2 and word in H().pmgt_last_error().decode()
    torch.cuda.synchronize()
    assert same_bits(s.p, p) and int(s.step[0]) == 0
    assert call(_lib.StepGuardC(P(s.counters), None, None, 0, None, 1)) == 0          # no log: both pointers may be NULL
    torch.cuda.synchronize()
    assert int(s.step[0]) == 1 and s.counters.tolist() == [1, 0, 0, 0]


# =========================================================================================== engine and trainer (golden model m1)
KW = dict(lr=1e-3, weight_decay=1e-2, max_grad_norm=5.0, scheduler_type="linear", num_warmup_steps=4, num_training_steps=20)


def trainer_on(case, dtype, **kw):
    from pmgt_amd.trainer import Trainer
    eng = make_engine(case, dtype=dtype, **NO_DROP)
    return eng, Trainer(eng, **dict(KW, **kw))


def grad_index(eng):
    return eng.entry("bert.encoder.layer.0.attention.self.query.weight")["offset"] + 5


def snapshot(eng):
    torch.cuda.synchronize()
    return dict(params=eng.params.clone(), exp_avg=eng.exp_avg.clone(), exp_avg_sq=eng.exp_avg_sq.clone(), opt_step=eng.opt_step.clone())


def assert_same(a, b):
    for k in a:
        assert same_bits(a[k], b[k]), k


def poisoned_step(tr, batch, value=math.inf):
    """One micro-batch whose gradient buffer gets `value` in one encoder weight before the optimizer runs."""
    tr.training_step(batch)
    tr.engine.grads[grad_index(tr.engine)] = value
    tr.optimizer_step()


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_eager_step_with_an_inf_gradient_is_skipped(dtype):
    case = gu.model_case("m1")
    batch = dev_batch(case["batch"])
    eng, tr = trainer_on(case, dtype, nonfinite="skip", step_log=4)
    tr.train_step(batch)                                   # one applied step: the moments are not zero, opt_step = 1
    before = snapshot(eng)
    poisoned_step(tr, batch)
    assert_same(before, snapshot(eng))
    assert int(eng.opt_step.item()) == 1 and eng.was_skipped().item() == 1.0 and math.isinf(eng.grad_norm().item())
    assert bool(torch.isfinite(eng.params).all())
    assert eng.step_counters() == {"attempts": 2, "skipped": 1, "skipped_in_a_row": 1}
    tr.train_step(batch)
    torch.cuda.synchronize()
    assert not torch.equal(eng.params, before["params"]) and bool(torch.isfinite(eng.params).all())
    assert int(eng.opt_step.item()) == 2 and eng.step_counters() == {"attempts": 3, "skipped": 1, "skipped_in_a_row": 0}
    # the rate of the UNSKIPPED position: linear warm-up 4, one step completed -> lr / 4; the skipped step consumed no warm-up
    assert eng.last_lr().item() == float(np.float32(float(np.float32(1e-3)) * 0.25))
    assert [(r["attempt"], r["opt_step"], r["skipped"]) for r in eng.step_log()] == [(0, 1, False), (1, 1, True), (2, 2, False)]
    # the same sequence without the guard: the parameters are lost -- the guarded run above guards something
    eng_u, tr_u = trainer_on(case, dtype)
    tr_u.train_step(batch)
    poisoned_step(tr_u, batch)
    torch.cuda.synchronize()
    assert not bool(torch.isfinite(eng_u.params).all()) and int(eng_u.opt_step.item()) == 2
    assert tr_u.check_nonfinite() is None                  # no guard, no counters to judge by


@pytest.mark.parametrize("guarding", [None, "skip"])
def test_step_log_ring_wraps_and_copies_the_steps_own_values(guarding):
    """6 eager steps into a ring of 4: attempts 2 .. 5 in order, each row the loss / norm / rate of its step bit for bit.  Alone
    (nonfinite=None) the log does not guard."""
    case = gu.model_case("m1")
    batch = dev_batch(case["batch"])
    eng, tr = trainer_on(case, "bf16", nonfinite=guarding, step_log=4)
    eng_plain, tr_plain = trainer_on(case, "bf16")
    seen = []
    for _ in range(6):
        loss = tr.train_step(batch).item()
        seen.append((loss, eng.grad_norm().item(), eng.last_lr().item(), eng._opt_scalars8[0].item()))
        tr_plain.train_step(batch)
    log = eng.step_log()
    assert [r["attempt"] for r in log] == [2, 3, 4, 5] and [r["opt_step"] for r in log] == [3, 4, 5, 6]
    for r, (loss, norm, lr, coef) in zip(log, seen[2:]):
        assert (r["loss"], r["grad_norm"], r["lr"], r["clip_coef"]) == (loss, norm, lr, coef) and not r["skipped"] and not r["nonfinite"]
    assert len({r["loss"] for r in log}) == 4 and all(math.isfinite(r["loss"]) for r in log)
    assert_same(snapshot(eng), snapshot(eng_plain))        # logging (and guarding good steps) changes no bit of the run
    assert eng.step_counters() == {"attempts": 6, "skipped": 0, "skipped_in_a_row": 0}


def poison_table(eng, batch):
    """Sets the feature row of the first target of `batch` to inf in table 0; returns restore()."""
    row = int(batch[0]["node_ids"][0, 0])
    saved = eng.tables[0][row].clone()
    eng.tables[0][row] = math.inf

    def restore():
        eng.tables[0][row] = saved
    return restore


def test_captured_step_skips_a_poisoned_replay():
    case = gu.model_case("m1")
    batch = dev_batch(case["batch"])
    eng, tr = trainer_on(case, "bf16", nonfinite="skip", step_log=4)
    # an eager step first: a referenced row of a frozen table at inf makes the gradient norm non-finite (and is skipped)
    restore = poison_table(eng, batch)
    tr.train_step(batch)
    assert not math.isfinite(eng.grad_norm().item())
    restore()
    assert eng.step_counters()["skipped"] == 1 and int(eng.opt_step.item()) == 0
    replay = tr.capture_step(batch, warmup=2)              # the capture succeeds: nothing in the guarded step breaks it
    s0 = snapshot(eng)
    assert int(s0["opt_step"]) == 2
    replay()
    s1 = snapshot(eng)
    restore = poison_table(eng, batch)
    replay()
    s2 = snapshot(eng)
    restore()
    assert_same(s1, s2)
    assert eng.step_counters() == {"attempts": 5, "skipped": 2, "skipped_in_a_row": 1}
    replay()
    s3 = snapshot(eng)
    assert bool(torch.isfinite(s3["params"]).all()) and not torch.equal(s3["params"], s2["params"]) and not torch.equal(s1["params"], s0["params"])
    assert int(s3["opt_step"]) == 4                        # advanced by 2 over the three replays
    log = eng.step_log()[-3:]
    assert [(r["attempt"], r["skipped"], r["opt_step"]) for r in log] == [(3, False, 3), (4, True, 3), (5, False, 4)]
    assert math.isfinite(log[0]["loss"]) and math.isfinite(log[2]["loss"]) and not math.isfinite(log[1]["grad_norm"])
    assert log[2]["loss"] == tr.last_loss.item()           # the capture's private loss scalar is what the log reads


def test_run_live_reports_losses_and_skips():
    from pmgt_amd.trainer import Trainer
    case = gu.model_case("m3")
    smp, ids = live_inputs(case, 128)
    eng = make_engine(case, dtype="bf16", **NO_DROP)
    tr = Trainer(eng, nonfinite="skip", step_log=8, **KW)
    res = tr.run_live(smp, ids, batch_size=32, steps=4, threads=2, depth=3, graphs=True)
    assert res["skipped_steps"] == 0 and len(res["loss_train"]) == 4 and all(math.isfinite(x) for x in res["loss_train"])
    assert res["loss_train"][-1] == tr.last_loss.item() and int(eng.opt_step.item()) == 4
    plain = Trainer(make_engine(case, dtype="bf16", **NO_DROP), **KW).run_live(smp, ids, batch_size=32, steps=2, threads=2, depth=3)
    assert "skipped_steps" not in plain and "loss_train" not in plain          # the unguarded trainer's result is what it was
    tr.drop_captured_steps()


def test_accumulation_window_after_a_skip_is_clean():
    """accumulate_grad_batches = 2: window 1 applied, window 2 poisoned after its second micro-batch (skipped), window 3.  Window 3 equals,
    bit for bit, the same window on a trainer that went from window 1 straight to it (with the dropout / masking counter of that point)."""
    case = gu.model_case("m1")
    batch = dev_batch(case["batch"])
    eng_a, tr_a = trainer_on(case, "bf16", nonfinite="skip", accumulate_grad_batches=2)
    eng_b, tr_b = trainer_on(case, "bf16", nonfinite="skip", accumulate_grad_batches=2)
    for tr in (tr_a, tr_b):
        tr.train_step(batch)
        tr.train_step(batch)
    after_1 = snapshot(eng_a)
    tr_a.train_step(batch)
    tr_a.training_step(batch)                              # the window's second micro-batch (accumulates), then the poison, then the step
    eng_a.grads[grad_index(eng_a)] = math.nan
    tr_a.optimizer_step()
    tr_a._micro = 0
    assert_same(after_1, snapshot(eng_a))
    assert eng_a.step_counters() == {"attempts": 2, "skipped": 1, "skipped_in_a_row": 1}
    eng_b.rng_state.copy_(eng_a.rng_state)
    for tr in (tr_a, tr_b):
        tr.train_step(batch)
        tr.train_step(batch)
    assert_same(snapshot(eng_a), snapshot(eng_b))
    assert int(eng_a.opt_step.item()) == 2 and not torch.equal(eng_a.params, after_1["params"])


def test_checkpoint_carries_counters_and_settings_and_resumes_bit_identically(tmp_path):
    from pmgt_amd import io as pio
    from pmgt_amd.trainer import Trainer
    case = gu.model_case("m1")
    batch = dev_batch(case["batch"])
    guard = dict(nonfinite="skip", step_log=4)

    def part_1(tr):
        tr.train_step(batch)
        poisoned_step(tr, batch)

    def part_2(tr):
        tr.train_step(batch)
        poisoned_step(tr, batch, math.nan)
        tr.train_step(batch)
    eng_a, tr_a = trainer_on(case, "bf16", **guard)
    part_1(tr_a)
    part_2(tr_a)
    eng_b, tr_b = trainer_on(case, "bf16", **guard)
    part_1(tr_b)
    ck = pio.save_training_checkpoint(eng_b, tr_b, tmp_path / "g.ckpt")
    assert ck["pmgt_amd"]["step_counters"] == {"attempts": 2, "skipped": 1, "skipped_in_a_row": 1}
    assert ck["pmgt_amd"]["hyper_parameters"]["nonfinite"] == "skip" and ck["pmgt_amd"]["hyper_parameters"]["step_log"] == 4
    assert ck["global_step"] == 1
    eng_c = fresh_engine(case, "bf16", seed=9, **NO_DROP)
    tr_c = Trainer(eng_c, **dict(KW, **guard))
    pio.load_training_checkpoint(eng_c, tr_c, str(tmp_path / "g.ckpt"))
    assert eng_c.step_counters() == {"attempts": 2, "skipped": 1, "skipped_in_a_row": 1} and eng_c.step_log() == []
    part_2(tr_c)
    assert_same(snapshot(eng_a), snapshot(eng_c))
    assert torch.equal(eng_a.rng_state, eng_c.rng_state)
    assert eng_c.step_counters() == eng_a.step_counters() == {"attempts": 5, "skipped": 2, "skipped_in_a_row": 0}
    assert [r["attempt"] for r in eng_c.step_log()] == [2, 3, 4]
    # a trainer with other settings: named like the other hyper-parameters
    eng_d = fresh_engine(case, "bf16", **NO_DROP)
    with pytest.raises(ValueError) as ei:
        pio.load_training_checkpoint(eng_d, Trainer(eng_d, **KW), str(tmp_path / "g.ckpt"))
    assert "nonfinite: checkpoint 'skip', trainer None" in str(ei.value) and "step_log: checkpoint 4, trainer 0" in str(ei.value)
    # a file from before the guard existed (no counters, neither setting): loads into a default trainer, the counters are zero
    old = copy.deepcopy(pio.read_checkpoint(str(tmp_path / "g.ckpt")))
    del old["pmgt_amd"]["step_counters"], old["pmgt_amd"]["hyper_parameters"]["nonfinite"], old["pmgt_amd"]["hyper_parameters"]["step_log"]
    eng_d.step_counters_dev.fill_(7)
    pio.load_training_checkpoint(eng_d, Trainer(eng_d, **KW), old)
    assert eng_d.step_counters() == {"attempts": 0, "skipped": 0, "skipped_in_a_row": 0}
    assert torch.equal(eng_d.params, eng_b.params)


def test_fit_stops_before_writing_a_checkpoint_and_logs_a_clean_run(tmp_path):
    """Every row of one frozen table at inf for the whole run (one row would not be in every random batch): every step is skipped, fit
    raises at the end of its first run of training steps, the parameters are the initial ones and no file exists.  Unpoisoned, the
    history carries skipped_steps = 0 and a finite loss/train per epoch."""
    from pmgt_amd.trainer import NonFiniteGradientsError, fit
    args = dict(batch_size=48, max_epochs=2, patience=5, seed=5, threads=2, valid_batch_size=32)
    eng, tr, smp, train_ids, valid_ids = fit_world()
    initial = eng.params.clone()
    eng.tables[0][2:] = math.inf
    with pytest.raises(NonFiniteGradientsError, match="3 optimizer steps in a row.*3 of 3 steps skipped") as ei:
        fit(tr, eng, smp, train_ids, valid_ids, ckpt_dir=str(tmp_path / "bad"), nonfinite="skip", step_log=8,
            max_skipped_in_a_row=3, **args)
    assert ei.value.counters == {"attempts": 3, "skipped": 3, "skipped_in_a_row": 3} and "last logged pre-clip norm" in str(ei.value)
    assert torch.equal(eng.params, initial) and bool(torch.isfinite(eng.params).all()) and int(eng.opt_step.item()) == 0
    assert os.listdir(tmp_path / "bad") == []
    eng, tr, smp, train_ids, valid_ids = fit_world()
    res = fit(tr, eng, smp, train_ids, valid_ids, ckpt_dir=str(tmp_path / "good"), nonfinite="skip", step_log=8, max_skipped_in_a_row=3, **args)
    assert len(res["history"]) == 2 and tr.nonfinite == "skip" and tr.step_log == 8
    for h in res["history"]:
        assert h["skipped_steps"] == 0 and math.isfinite(h["loss/train"]) and math.isfinite(h["loss/val"])
    assert int(eng.opt_step.item()) == 8 and sorted(os.listdir(tmp_path / "good"))[-1] == "last.ckpt"
