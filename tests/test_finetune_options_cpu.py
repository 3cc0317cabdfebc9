"""What the fine-tune run's options rest on that needs no GPU: the library exports pmgt_op_step_segments and the binding states the header's
declaration; the comparison of a last.ckpt's run record against a call names both values; the schedule lengths fit_pmgt_ncf computes are
pair_schedule_steps', the reference's (N + B - 1) // B * epochs with int(warmup * total) (pmgt/base_trainer.py:71-90)."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from pmgt_amd import _build, _lib
from pmgt_amd.pair_train import check_run_record, pair_schedule_steps, pair_trainer_options, run_record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_pmgt_op_step_segments():
    out = subprocess.run(["nm", "-D", _build.hip_lib_path()], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert "pmgt_op_step_segments" in names and "pmgt_op_adamw_segments" in names
    assert "pmgt_op_step_segments" in _lib.OPS_SYMBOLS
    assert os.path.join(os.path.dirname(_build.__file__), "ops", "segments_step.hip") in _build.OPS_SOURCES


def test_header_constants_and_binding_agree():
    hdr = open(os.path.join(ROOT, "include", "pmgt_ops.h")).read()
    defines = dict(re.findall(r"#define (PMGT_OPTIM_\w+)\s+(\d+)", hdr))
    assert {k: int(v) for k, v in defines.items()} == {"PMGT_OPTIM_ADAMW": _lib.OPTIMS.index("adamw"), "PMGT_OPTIM_SGD": _lib.OPTIMS.index("sgd")}
    assert int(re.search(r"#define PMGT_ADAM_MAX_SEGMENTS (\d+)", hdr).group(1)) == _lib.ADAM_MAX_SEGMENTS
    decl = re.search(r"int pmgt_op_step_segments\((.*?)\);", hdr, re.S).group(1)
    params = [" ".join(p.split()) for p in decl.split(",")]
    assert params == ["const pmgt_adam_segment* segments", "int count", "int optim", "float lr", "float wd", "float b1", "float b2", "float eps",
                      "float max_norm", "int64_t* step", "float* scal", "float* part", "const pmgt_lr_schedule* sched",
                      "const pmgt_step_guard* guard", "void* stream"]
    f, vp = C.c_float, C.c_void_p
    want = [C.POINTER(_lib.AdamSegmentC), C.c_int, C.c_int] + [f] * 6 + [vp] * 3 + [C.POINTER(_lib.LrScheduleC), C.POINTER(_lib.StepGuardC), vp]
    src = inspect.getsource(_lib)
    bound = re.search(r"L\.pmgt_op_step_segments\.argtypes = \[(.*?)\]", src, re.S).group(1)
    ns = dict(C=C, i=C.c_int, i64=C.c_int64, f=f, vp=vp, AdamSegmentC=_lib.AdamSegmentC, LrScheduleC=_lib.LrScheduleC, StepGuardC=_lib.StepGuardC)
    assert eval("[" + bound + "]", ns) == want and len(want) == len(params)
    # the old entry's declaration is what it was: the same list without optim, sched and guard
    old = [" ".join(p.split()) for p in re.search(r"int pmgt_op_adamw_segments\((.*?)\);", hdr, re.S).group(1).split(",")]
    assert old == [p for p in params if p.split()[-1] not in ("optim", "sched", "guard")]


class _Trainer:
    def __init__(self, schedule):
        self._schedule = schedule

    def schedule(self):
        return self._schedule


def test_resume_comparison_names_both_values():
    call = dict(batch_size=32, num_ng=1, seed=3, early_criterion="n20", patience=10, max_epochs=4)
    plain, scheduled = run_record(_Trainer(None), **call), run_record(_Trainer(("linear", 1, 40)), **call)
    assert plain == {k: v for k, v in call.items() if k != "max_epochs"} and scheduled == call      # max_epochs only sets a schedule's length
    check_run_record("fit_pmgt_ncf", dict(scheduled), scheduled)
    check_run_record("fit_pmgt_ncf", dict(scheduled), plain)                 # (a recorded max_epochs binds a scheduled call only)
    for key, other in (("batch_size", 64), ("num_ng", 2), ("seed", 4), ("early_criterion", "loss"), ("patience", 2), ("max_epochs", 5)):
        with pytest.raises(ValueError, match=rf"fit_pmgt_ncf\(resume_from=\.\.\.\).*written with {key} = {other!r}, this call has {call[key]!r}"):
            check_run_record("fit_pmgt_ncf", dict(scheduled, **{key: other}), scheduled)
    with pytest.raises(ValueError, match=r"written with max_epochs = None, this call has 4"):
        check_run_record("fit_pmgt_ncf", plain, scheduled)                   # written without a schedule, resumed with one


@pytest.mark.parametrize("n_pos,num_ng,batch,epochs,warmup", [(58, 1, 32, 4, 0.1), (1000, 4, 256, 7, 0.06), (31, 0, 32, 3, None), (33, 0, 32, 3, 0.5)])
def test_schedule_lengths_are_the_references_formula(n_pos, num_ng, batch, epochs, warmup):
    rows = n_pos * (1 + num_ng)
    total = (rows + batch - 1) // batch * epochs             # the reference's formula on the epoch's actual number of rows
    want = (total, 0 if warmup is None else int(warmup * total))
    assert pair_schedule_steps(n_pos, num_ng, batch, epochs, warmup) == want
    opts = pair_trainer_options("fit_pmgt_ncf", n_pos, num_ng, batch, epochs, optim="sgd", scheduler_type="linear", scheduler_warmup=warmup,
                                nonfinite="skip", step_log=8)
    assert opts == dict(optim="sgd", nonfinite="skip", step_log=8, scheduler_type="linear", num_warmup_steps=want[1], num_training_steps=want[0])
    # the steps of an epoch as fit_pmgt_ncf's loop counts them
    assert total // epochs == (n_pos * (1 + int(num_ng)) + int(batch) - 1) // int(batch)
    assert "scheduler_type" not in pair_trainer_options("fit_pmgt_ncf", n_pos, num_ng, batch, epochs)
    with pytest.raises(ValueError, match="fit_pmgt_ncf: scheduler_warmup"):
        pair_trainer_options("fit_pmgt_ncf", n_pos, num_ng, batch, epochs, scheduler_warmup=0.1)


def test_fit_and_trainer_take_the_keywords_with_todays_defaults():
    from pmgt_amd.finetune import PmgtNcfOptionsTrainer, PmgtNcfTrainer, fit_pmgt_ncf
    plain, sig = inspect.signature(PmgtNcfTrainer.__init__).parameters, inspect.signature(PmgtNcfOptionsTrainer.__init__).parameters
    options = dict(optim="adamw", scheduler_type=None, num_warmup_steps=None, num_training_steps=None, nonfinite=None, step_log=0,
                   max_skipped_in_a_row=25)
    assert {k: sig[k].default for k in options} == options
    # the options trainer adds the keywords and nothing else: the plain trainer's list, with its defaults, comes first
    assert list(sig)[:len(plain)] == list(plain) and list(sig)[len(plain):] == list(options) and not set(options) & set(plain)
    assert all(sig[k].default == plain[k].default for k in plain) and issubclass(PmgtNcfOptionsTrainer, PmgtNcfTrainer)
    sig = inspect.signature(fit_pmgt_ncf).parameters
    assert {k: sig[k].default for k in ("optim", "scheduler_type", "scheduler_warmup", "nonfinite", "step_log", "save_last", "resume_from",
                                        "graph")} == dict(optim="adamw", scheduler_type=None, scheduler_warmup=None, nonfinite=None, step_log=0,
                                                          save_last=False, resume_from=None, graph=False)
