"""The layout of the pair heads' training after it got one home (pmgt_amd/pair_train.py), no GPU: the trainer and gradient-wrapper methods exist
once, in the bases; every name that moved is the same object at its old path(s); the module loads no GPU library; and the refusals the two heads
share differ in the head's name alone.  Identities and strings: comparisons are exact."""
import importlib
import os
import subprocess
import sys

import pytest

from pmgt_amd import dcn_head, ncf_head, pair_train

ncf_train = importlib.import_module("pmgt_amd.ncf_train")
dcn_train = importlib.import_module("pmgt_amd.dcn_train")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAINER_METHODS = ("views", "step", "_logits", "capture", "replay", "state_dict", "load_state_dict")
# name in pair_train -> (module, name there) of every old path
MOVED = {"ng_sample": [(ncf_train, "ng_sample"), (dcn_train, "ng_sample")],
         "normalize_item_table": [(ncf_train, "normalize_item_table"), (dcn_train, "normalize_item_table")],
         "check_ids": [(ncf_head, "check_ids"), (dcn_head, "check_ids"), (dcn_train, "check_ids")],
         "head_weights": [(ncf_head, "head_weights"), (dcn_head, "head_weights")],
         "_fmix32": [(ncf_head, "_fmix32")],
         "check_pairs": [(ncf_head, "check_pairs"), (ncf_train, "check_pairs"), (dcn_head, "check_pairs")],
         "check_dropout_p": [(ncf_head, "check_dropout_p"), (ncf_train, "check_dropout_p")],
         "dropout_keep": [(ncf_head, "ncf_dropout_keep"), (ncf_train, "ncf_dropout_keep"), (dcn_head, "ncf_dropout_keep")],
         "dropout_scale": [(ncf_head, "ncf_dropout_scale"), (dcn_head, "ncf_dropout_scale")],
         "bce_with_logits_host": [(dcn_train, "bce_with_logits_host")]}


def test_the_trainer_methods_exist_once():
    assert issubclass(ncf_train.NcfHeadTrainer, pair_train.PairTrainer) and issubclass(dcn_train.DcnTrainer, pair_train.PairTrainer)
    for name in TRAINER_METHODS:
        assert name not in vars(ncf_train.NcfHeadTrainer) and name not in vars(dcn_train.DcnTrainer), name
        assert name in vars(pair_train.PairTrainer), name


def test_the_wrapper_methods_exist_once():
    assert issubclass(ncf_train.NcfHeadGrad, pair_train.PairGrad) and issubclass(dcn_train.DcnGrad, pair_train.PairGrad)
    for name in ("reserve", "__call__"):
        assert name in vars(pair_train.PairGrad), name
        assert name not in vars(ncf_train.NcfHeadGrad) and name not in vars(dcn_train.DcnGrad), name
    assert "forward" in vars(dcn_train.DcnGrad) and not hasattr(pair_train.PairGrad, "forward")


def test_every_moved_name_is_the_same_object_at_its_old_paths():
    for name, olds in MOVED.items():
        home = getattr(pair_train, name)
        assert home.__module__ == "pmgt_amd.pair_train", name
        for mod, old in olds:
            assert getattr(mod, old) is home, (mod.__name__, old)
    assert ncf_head.ncf_dropout_keep is pair_train.dropout_keep
    assert dcn_train.ng_sample is ncf_train.ng_sample is pair_train.ng_sample
    import pmgt_amd
    assert pmgt_amd.ng_sample is pair_train.ng_sample and pmgt_amd.ncf_dropout_keep is pair_train.dropout_keep
    assert pmgt_amd.normalize_item_table is pair_train.normalize_item_table


def test_the_module_imports_without_a_gpu_library():
    code = ("import pmgt_amd.pair_train; "
            "assert 'libpmgt_hip' not in open('/proc/self/maps').read(); print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def _message(call):
    with pytest.raises(ValueError) as err:
        call()
    return str(err.value)


def test_the_shared_refusals_differ_in_the_heads_name_alone():
    tail = "emb_dropout = 1.0 outside [0, 1)"
    assert _message(lambda: pair_train.check_dropout_p(1.0, "emb_dropout")) == "ncf_train: " + tail
    assert _message(lambda: dcn_head.check_dcn_p(1.0, "emb_dropout")) == "dcn: " + tail
    assert pair_train.check_dropout_p(0.25, "p") == dcn_head.check_dcn_p(0.25, "p") == 0.25
    tail = "users in [0, 5] outside [0, 5)"
    assert _message(lambda: pair_train.check_pairs([0, 5], [0, 0], [1.0, 0.0], 5, 9)) == "ncf_train: " + tail
    assert _message(lambda: dcn_head.check_dcn_pairs([0, 5], [0, 0], [1.0, 0.0], 5, 9)) == "dcn: " + tail
    for seed in (True, 1.5, "7", 2 ** 63):
        assert _message(lambda: pair_train.check_seed(seed, "dcn")) == f"dcn: dropout_seed = {seed!r} must be an integer that fits int64"
    assert pair_train.check_seed(-2 ** 63, "dcn") == -2 ** 63


def test_per_layer_repeats_a_scalar_and_refuses_a_list_of_another_length_in_the_words_of_its_four_sites():
    assert pair_train.per_layer(0.5, 3, "unused", "anyone") == [0.5, 0.5, 0.5]
    assert pair_train.per_layer((0.1, 0.2), 2, "unused", "anyone") == [0.1, 0.2]
    ncf = "ncf_train: 2 layer dropouts for 3 layers"
    assert _message(lambda: pair_train.per_layer([0.1, 0.2], 3, ncf_head.LAYER_DROPOUTS, "ncf_train")) == ncf
    assert _message(lambda: ncf_head.ncf_dropout_masks(1, 0, 4, 8, 3, "MLP", 0.1, [0.1, 0.2])) == ncf
    dcn = "dcn: 2 deep and 2 cross dropouts for 2 deep and 3 cross layers"      # one refusal names both lists, the scalar one at its full length
    assert _message(lambda: dcn_head.dcn_per_layer(0.0, [0.1, 0.2], 2, 3)) == dcn
    assert _message(lambda: dcn_head.dcn_dropout_masks(1, 0, 4, 8, 2, 3, 0.1, 0.0, [0.1, 0.2])) == dcn
    assert dcn_head.dcn_per_layer(0.3, [0.1, 0.2, 0.0], 2, 3) == ([0.3, 0.3], [0.1, 0.2, 0.0])
