"""The layout of the training surface after its split by concern (pmgt_amd/trainer.py, pipeline.py, evaluation.py, fit_loop.py), no GPU: the
old import path of every public name, the one definition of the guard settings and of the step's frozen settings, the two named predicates
and the batch-to-device helper.  Identities, strings and small integers: comparisons are exact."""
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from pmgt_amd import evaluation, fit_loop, pipeline, trainer
from pmgt_amd.trainer import Trainer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOMES = {pipeline: ("PipelineError", "ProducerPipeline"),
         evaluation: ("roc_auc_score", "EVAL_PINNED_SLOTS", "evaluate", "export_embeddings"),
         fit_loop: ("monitor_of", "EarlyStopping", "BestCheckpoint", "epoch_order", "fit")}
BAD_GUARDS = (dict(nonfinite="drop"), dict(step_log=-1), dict(max_skipped_in_a_row=0))


def test_every_public_name_is_still_importable_from_trainer_and_is_the_object_of_its_new_module():
    assert trainer.Trainer.__module__ == trainer.NonFiniteGradientsError.__module__ == "pmgt_amd.trainer"
    for home, names in HOMES.items():
        for name in names:
            assert getattr(trainer, name) is getattr(home, name), name
            if name != "EVAL_PINNED_SLOTS":
                assert getattr(home, name).__module__ == home.__name__, name


def test_fit_loop_imports_without_the_trainer_module_and_without_a_gpu_library():
    code = ("import sys; import pmgt_amd.fit_loop; "
            "assert 'pmgt_amd.trainer' not in sys.modules; "
            "assert 'pmgt_amd.engine' not in sys.modules; "
            "assert 'libpmgt_hip' not in open('/proc/self/maps').read(); print('ok')")      # (the bindings module alone loads nothing)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def _message(call):
    with pytest.raises(ValueError) as err:
        call()
    return str(err.value)


@pytest.mark.parametrize("bad", BAD_GUARDS, ids=lambda b: next(iter(b)))
def test_constructor_set_guard_and_fit_refuse_a_bad_guard_setting_in_the_same_words(bad):
    want = _message(lambda: Trainer(None, **bad))
    (name, value), = bad.items()
    assert f"{name}={value!r}" in want
    tr = Trainer(None, nonfinite="skip", step_log=4)
    assert _message(lambda: tr.set_guard(**bad)) == want
    # fit passes the value through set_guard before it touches the engine (there is none: the trainer drives None, and None is passed)
    assert _message(lambda: fit_loop.fit(tr, None, None, np.arange(4), np.arange(4), batch_size=2, max_epochs=1, **bad)) == want
    assert (tr.nonfinite, tr.step_log, tr.max_skipped_in_a_row) == ("skip", 4, 25)      # a refused call assigns nothing


def test_set_guard_assigns_what_is_passed_and_keeps_the_rest():
    tr = Trainer(None, nonfinite="skip", step_log=4, max_skipped_in_a_row=7)
    tr.set_guard(step_log="16")
    assert (tr.nonfinite, tr.step_log, tr.max_skipped_in_a_row) == ("skip", 16, 7) and isinstance(tr.step_log, int)
    tr.set_guard(nonfinite=None, max_skipped_in_a_row=3)
    assert (tr.nonfinite, tr.step_log, tr.max_skipped_in_a_row) == (None, 16, 3)
    tr.set_guard()
    assert (tr.nonfinite, tr.step_log, tr.max_skipped_in_a_row) == (None, 16, 3)
    with pytest.raises(TypeError):
        tr.set_guard(lr=1e-3)


def test_the_frozen_settings_are_listed_once_by_name_in_the_order_of_the_key():
    tr = Trainer(None, lr=2e-3, weight_decay=0.05, betas=[0.8, 0.95], eps=1e-6, max_grad_norm=5, random_node_ratio=0.03, mask_node_ratio=0.2,
                 nonfinite="skip", step_log=16, scheduler_type="cosine", num_warmup_steps=2, num_training_steps=10)
    hp = tr.hyper_parameters()
    assert list(hp) == ["lr", "weight_decay", "betas", "eps", "max_grad_norm", "random_node_ratio", "mask_node_ratio", "nonfinite", "step_log",
                        "schedule"]
    assert tr._hyper_key() == tuple(hp.values()) == (2e-3, 0.05, (0.8, 0.95), 1e-6, 5.0, 0.03, 0.2, "skip", 16, ("cosine", 2, 10))
    assert isinstance(hp["betas"], tuple) and isinstance(hp["max_grad_norm"], float) and tr._capture_key() == tr._hyper_key()
    plain = Trainer(None)
    assert plain._hyper_key() == (1e-3, 1e-2, (0.9, 0.999), 1e-8, None, 0.02, 0.16, None, 0, None)
    assert not hasattr(Trainer, "HYPER_NAMES")


@pytest.mark.parametrize("world_size,accum,force", list(itertools.product((1, 2), (1, 2), (False, True))))
def test_the_two_predicates_of_the_step(world_size, accum, force):
    tr = Trainer(None, world_size=world_size, accumulate_grad_batches=accum, force_exchange=force, overlap_allreduce=False)
    assert tr._exchanging is (world_size > 1 or force)
    assert tr._capturable is (world_size == 1 and accum == 1 and not force)
    with pytest.raises(AttributeError):
        tr._capturable = True
    if not tr._capturable:
        with pytest.raises(AssertionError, match="capture covers the single-GPU, non-accumulating step"):
            tr.capture_step(None)


def test_batch_to_device_keeps_the_layout_of_a_sampler_batch():
    g = torch.Generator().manual_seed(0)
    ids = lambda *shape: torch.randint(0, 50, shape, generator=g)
    batch = ({"node_ids": ids(3, 4), "attention_mask": torch.ones(3, 4)}, {"node_ids": ids(6, 4), "attention_mask": torch.ones(6, 4)},
             torch.tensor([2, 2, 2]), torch.tensor([1., 0., 1., 0., 1., 0.]))
    for non_blocking in (False, True):
        got = evaluation.batch_to_device(batch, "cpu", non_blocking=non_blocking)
        assert isinstance(got, tuple) and len(got) == 4
        for a, b in zip(got[:2], batch[:2]):
            assert list(a) == list(b) and all(torch.equal(a[k], b[k]) and a[k].dtype == b[k].dtype for k in b)
        assert torch.equal(got[2], batch[2]) and torch.equal(got[3], batch[3])
