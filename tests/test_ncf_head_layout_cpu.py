"""The layout of the NCF head after it got one home (pmgt_amd/ncf_head.py, the bindings in pmgt_amd/_lib.py), no GPU: the old import path of
every name that moved, the constants against the #defines of include/pmgt_capi.h, the one stream helper, and the refusals that several
entry points now share word for word.  Identities, strings and small integers: comparisons are exact."""
import importlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from pmgt_amd import _lib, averaging, engine, evaluation, metrics, ncf_head

recommend_mod = importlib.import_module("pmgt_amd.recommend")      # (pmgt_amd.recommend, the attribute, is the function)
ncf_train = importlib.import_module("pmgt_amd.ncf_train")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_NAMES = {recommend_mod: ("head_shape", "check_head_covered", "ncf_head_host"),
              ncf_train: ("HEAD_PREFIXES", "TABLE_KEY", "head_layout", "table_layout", "layout_slots", "check_pairs", "ncf_head_grad_host",
                          "head_state")}
LIB_NAMES = {recommend_mod: ("NCF_MAX_LAYERS", "NCF_MAX_USERS", "NCF_FACTORS", "NCF_MAX_D", "TOPK_MAX_K", "TOPK_FLAG_NAN", "TOPK_FLAG_SHORT"),
             ncf_train: ("NcfTrainC", "NCF_TRAIN_MAX_PAIRS", "NCF_TRAIN_TENSORS")}


def test_every_moved_name_is_still_importable_from_its_old_module_and_is_the_object_of_its_new_home():
    for old, names in HEAD_NAMES.items():
        for name in names:
            assert getattr(old, name) is getattr(ncf_head, name), name
            if callable(getattr(ncf_head, name)):      # (check_pairs moved on to pair_train.py, which both pair heads share)
                assert getattr(ncf_head, name).__module__ == ("pmgt_amd.pair_train" if name == "check_pairs" else "pmgt_amd.ncf_head"), name
    for old, names in LIB_NAMES.items():
        for name in names:
            assert getattr(old, name) is getattr(_lib, name), name
    assert _lib.NcfTrainC.__module__ == _lib.NcfHeadC.__module__ == "pmgt_amd._lib"
    assert ncf_head.check_ids.__module__ == "pmgt_amd.pair_train" and ncf_head.check_item_table.__module__ == "pmgt_amd.ncf_head"


def test_the_head_module_imports_without_a_gpu_library():
    code = ("import pmgt_amd.ncf_head; "
            "assert 'libpmgt_hip' not in open('/proc/self/maps').read(); print('ok')")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_the_mirrored_constants_equal_the_defines_of_the_header():
    text = open(os.path.join(ROOT, "include", "pmgt_capi.h")).read()
    defines = {name: int(value) for name, value in re.findall(r"^#define (PMGT_(?:NCF|TOPK)_\w+) (\d+)u?$", text, re.M)}
    assert defines == {"PMGT_NCF_MLP": _lib.NCF_KINDS.index("MLP"), "PMGT_NCF_NEUMF_END": _lib.NCF_KINDS.index("NeuMF-end"),
                       "PMGT_NCF_MAX_LAYERS": _lib.NCF_MAX_LAYERS, "PMGT_NCF_MAX_USERS": _lib.NCF_MAX_USERS,
                       "PMGT_NCF_TRAIN_MAX_PAIRS": _lib.NCF_TRAIN_MAX_PAIRS, "PMGT_NCF_TRAIN_TENSORS": _lib.NCF_TRAIN_TENSORS,
                       "PMGT_TOPK_MAX_K": _lib.TOPK_MAX_K, "PMGT_TOPK_FLAG_NAN": _lib.TOPK_FLAG_NAN, "PMGT_TOPK_FLAG_SHORT": _lib.TOPK_FLAG_SHORT}
    assert len(_lib.NCF_KINDS) == 2
    assert _lib.NcfHeadC.weight.size == _lib.NcfHeadC.bias.size == _lib.NCF_MAX_LAYERS * 8      # const float* [PMGT_NCF_MAX_LAYERS]


@pytest.mark.parametrize("kind", _lib.NCF_KINDS)
def test_the_tensor_count_is_the_slot_count(kind):
    layout, _ = ncf_head.head_layout(8, 2, kind, 3, 4)
    assert _lib.NCF_TRAIN_TENSORS == 3 + 2 * _lib.NCF_MAX_LAYERS + 2 == len(ncf_head.layout_slots(layout))
    assert len(ncf_head.layout_slots(ncf_head.table_layout(8, 2, kind, 3, 4)[0])) == _lib.NCF_TRAIN_TENSORS      # the table has no slot


def test_one_stream_helper():
    for mod in (engine, metrics, recommend_mod, ncf_train):
        assert not hasattr(mod, "_stream"), mod.__name__
    assert not hasattr(averaging.WeightAverage, "_stream") and callable(_lib.stream)


def _message(call):
    with pytest.raises(ValueError) as err:
        call()
    return str(err.value)


class FakeModel:
    """What recommend, evaluate_ranking, NcfHeadTrainer and fit_ncf read of a PMGT_NCF before they touch a device (it has no engine and no
    parameters: going further is an AttributeError, not the ValueError these tests expect)."""
    user_num, item_num, factor_num, num_layers, model = 5, 9, 16, 3, "MLP"
    mlp_layers = ()

    class emb_dropout:
        p = 0.0


@pytest.mark.parametrize("factor,layers,kind", [(12, 2, "MLP"), (64, 4, "MLP"), (8, 5, "NeuMF-end"), (8, 2, "GMF")])
def test_an_uncovered_head_is_refused_in_the_same_words_everywhere(factor, layers, kind):
    want = _message(lambda: ncf_head.check_head_covered(factor, layers, kind))
    assert want.startswith("ncf head: ")
    m = FakeModel()
    m.factor_num, m.num_layers, m.model = factor, layers, kind
    assert _message(lambda: ncf_head.head_layout(factor, layers, kind, 3, 4)) == want
    assert _message(lambda: ncf_head.table_layout(factor, layers, kind, 3, 4)) == want
    assert _message(lambda: recommend_mod.recommend(m, None, users=[0])) == want
    assert _message(lambda: ncf_train.NcfHeadTrainer(m, None)) == want


@pytest.mark.parametrize("bad", [5, -1])
def test_a_user_id_outside_the_table_is_refused_in_the_same_words_before_any_device_work(bad):
    m = FakeModel()
    tail = f": users in [{min(bad, 0)}, {max(bad, 0)}] outside [0, 5)"
    users = np.array([0, bad])
    cands = (np.zeros((2, 3), np.int64), np.ones((2, 3), np.float32), np.full(2, 3, np.int32))
    assert _message(lambda: ncf_head.check_ids("users", users, 5, "anyone")) == "anyone" + tail
    assert _message(lambda: ncf_head.check_pairs(users, [0, 0], [1.0, 0.0], 5, 9)) == "ncf_train" + tail
    assert _message(lambda: recommend_mod.recommend(m, None, users=users)) == "recommend" + tail
    assert _message(lambda: recommend_mod.exclusion_csr([(0, 0), (bad, 0)], 5, 9)) == "exclude" + tail
    for how in ("host", "device"):
        assert _message(lambda: evaluation.evaluate_ranking(m, None, users, *cands, metrics=how)) == "evaluate_ranking" + tail
    assert _message(lambda: evaluation.check_candidates(m, users, *cands, "anyone")) == "anyone" + tail
    assert _message(lambda: ncf_train.fit_ncf(m, None, [(0, 0)], (users, *cands), batch_size=2, max_epochs=1)) == "fit_ncf: validation" + tail
    # the training pairs go through check_pairs
    assert _message(lambda: ncf_train.fit_ncf(m, None, [(0, 0), (bad, 0)], (users, *cands), batch_size=2, max_epochs=1)) == "ncf_train" + tail
