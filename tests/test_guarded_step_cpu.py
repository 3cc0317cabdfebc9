"""Host side of the guarded optimizer step (pmgt_amd/trainer.py, pmgt_amd/io.py, pmgt_amd/_lib.py), no GPU: the two settings as
hyper-parameters, the checkpoint's counters and its backward compatibility, the skip policy of check_nonfinite on scripted counters, and
the C struct's layout.  Integer bookkeeping and copies: comparisons are exact."""
import ctypes as C

import pytest

from pmgt_amd import _lib
from pmgt_amd import io as pio
from pmgt_amd.trainer import NonFiniteGradientsError, Trainer
from tests.test_checkpoint_state_cpu import HP, make_entries, trainer_sd, weights_of


class ScriptedEngine:
    """step_counters() / step_log() as Engine has them, from a script."""

    def __init__(self, counters, log=()):
        self.counters, self.log, self.reads = dict(counters), list(log), 0

    def step_counters(self):
        self.reads += 1
        return dict(self.counters)

    def step_log(self):
        return list(self.log)


def test_settings_are_hyper_parameters_and_off_by_default():
    tr = Trainer(None, lr=1e-3)
    assert tr.nonfinite is None and tr.step_log == 0 and tr.max_skipped_in_a_row == 25 and tr._guard() is None
    hp = tr.hyper_parameters()
    assert hp["nonfinite"] is None and hp["step_log"] == 0 and list(hp)[-1] == "schedule"
    on = Trainer(None, lr=1e-3, nonfinite="skip", step_log=16)
    assert on.hyper_parameters()["nonfinite"] == "skip" and on.hyper_parameters()["step_log"] == 16
    assert on._hyper_key() != tr._hyper_key() and Trainer(None, lr=1e-3, step_log=16)._hyper_key() != on._hyper_key()
    assert on._guard() == dict(skip_nonfinite=True, log_rows=16, loss=None)
    assert Trainer(None, step_log=4)._guard() == dict(skip_nonfinite=False, log_rows=4, loss=None)      # logging alone does not guard
    for bad in (dict(nonfinite="raise"), dict(step_log=-1), dict(max_skipped_in_a_row=0)):
        with pytest.raises(ValueError):
            Trainer(None, **bad)


def test_mismatches_name_the_settings_and_an_older_file_means_off():
    on = Trainer(None, nonfinite="skip", step_log=8)
    off = Trainer(None)
    sd_on = {"hyper_parameters": on.hyper_parameters(), "accumulate_grad_batches": 1}
    assert on.hyper_mismatches(sd_on) == []
    assert off.hyper_mismatches(sd_on) == [("nonfinite", "skip", None), ("step_log", 8, 0)]
    older = {"hyper_parameters": {k: v for k, v in off.hyper_parameters().items() if k not in ("nonfinite", "step_log")},
             "accumulate_grad_batches": 1}
    assert off.hyper_mismatches(older) == []
    assert on.hyper_mismatches(older) == [("nonfinite", None, "skip"), ("step_log", 0, 8)]
    # a checkpoint of the reference records neither these nor a schedule: the trainer keeps its own
    assert on.hyper_mismatches({"hyper_parameters": {"lr": 1e-3, "weight_decay": 1e-2}}) == []


def test_checkpoint_carries_the_counters_and_an_older_one_has_none():
    entries, n = make_entries()
    sd = trainer_sd(entries, n, hp=dict(HP, nonfinite="skip", step_log=4))
    sd["engine"]["step_counters"] = {"attempts": 9, "skipped": 2, "skipped_in_a_row": 1}
    ck = pio.training_checkpoint(weights_of(entries, sd["engine"]["params"]), entries, sd)
    assert ck["pmgt_amd"]["step_counters"] == {"attempts": 9, "skipped": 2, "skipped_in_a_row": 1} and ck["global_step"] == 7
    back = pio.training_state_from_checkpoint(ck, entries, n)
    assert back["engine"]["step_counters"] == {"attempts": 9, "skipped": 2, "skipped_in_a_row": 1}
    assert back["hyper_parameters"]["nonfinite"] == "skip" and back["hyper_parameters"]["step_log"] == 4
    del ck["pmgt_amd"]["step_counters"]
    assert pio.training_state_from_checkpoint(ck, entries, n)["engine"]["step_counters"] == {}           # Engine.load_training_state: zeros
    plain = trainer_sd(entries, n)                                                                       # a state without counters
    assert pio.training_checkpoint(weights_of(entries, plain["engine"]["params"]), entries, plain)["pmgt_amd"]["step_counters"] == \
        {"attempts": 0, "skipped": 0, "skipped_in_a_row": 0}


def test_check_nonfinite_raises_at_the_limit_and_names_counts_and_norm():
    eng = ScriptedEngine({"attempts": 40, "skipped": 7, "skipped_in_a_row": 2},
                         [dict(attempt=39, opt_step=33, loss=1.0, grad_norm=float("inf"), clip_coef=0.0, lr=1e-3, skipped=True, nonfinite=True)])
    tr = Trainer(eng, nonfinite="skip", step_log=4, max_skipped_in_a_row=3)
    assert tr.check_nonfinite() == eng.counters and eng.reads == 1
    assert tr.check_nonfinite({"attempts": 1, "skipped": 0, "skipped_in_a_row": 0})["attempts"] == 1 and eng.reads == 1      # no second read
    eng.counters["skipped_in_a_row"] = 3
    with pytest.raises(NonFiniteGradientsError) as ei:
        tr.check_nonfinite()
    msg = str(ei.value)
    assert "last 3 optimizer steps in a row" in msg and "7 of 40 steps skipped" in msg and "inf (attempt 39)" in msg
    assert ei.value.counters == eng.counters and isinstance(ei.value, RuntimeError)
    eng.log = []
    with pytest.raises(NonFiniteGradientsError, match="not logged"):
        tr.check_nonfinite()
    # logging alone never raises; no guard: nothing is read
    assert Trainer(eng, step_log=4, max_skipped_in_a_row=1).check_nonfinite() == eng.counters
    reads = eng.reads
    assert Trainer(eng).check_nonfinite() is None and eng.reads == reads


def test_struct_layout_and_symbols():
    """pmgt_step_guard of include/pmgt_capi.h: three pointers, int64 log_rows, a pointer, an int (padded to 8)."""
    assert [f[0] for f in _lib.StepGuardC._fields_] == ["counters", "log_f", "log_i", "log_rows", "loss", "skip_nonfinite"]
    assert C.sizeof(_lib.StepGuardC) == 48 and _lib.StepGuardC.log_rows.offset == 24 and _lib.StepGuardC.skip_nonfinite.offset == 40
    assert "pmgt_optimizer_step_guarded" in _lib.HIP_SYMBOLS and "pmgt_op_adamw_guarded" in _lib.OPS_SYMBOLS
    assert _lib.STEP_LOG_FLOATS == 8
