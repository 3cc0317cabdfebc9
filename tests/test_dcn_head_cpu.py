"""The Deep & Cross Network on the host, no GPU: the numpy yardstick dcn_head_grad_host and the torch module dcn.DCN against the reference's
own model in fp64 (tests/golden/dcn_grad.npz, made by tests/golden/make_dcn_golden.py), the decay rule against the reference's
optimizer groups, the flat layout against the header, every refusal, and ng_sample as DCNDataset labels its pairs.

Tolerance: fp64 against fp64 of the same formula in another order of sums: 1e-12 absolute on the loss, the logits and every gradient.  The
DEGENERATE tensors (with LayerNorm: every cross weight, gamma / beta of every cross layer but the last; exactly 0 in exact arithmetic, 1e-10
to 1e-50 in the fixture) are judged absolutely against the largest non-degenerate gradient of the case, 1e-12 of it, not relatively."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.dcn import DCN
from pmgt_amd.dcn_head import (check_dcn_covered, check_dcn_dropout, check_dcn_pairs, dcn_head_grad_host, dcn_head_host, dcn_layout,
                               dcn_layout_slots, dcn_shape, decays)
from pmgt_amd.ncf_train import ng_sample
from tests.dcn_util import degenerate_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "dcn_grad.npz"))
TAGS = ("ln", "noln", "run")


def fixture(tag):
    w = {k[len(tag) + 3:]: GOLD[k] for k in GOLD.files if k.startswith(tag + "/w/")}
    g = {k[len(tag) + 3:]: GOLD[k] for k in GOLD.files if k.startswith(tag + "/g/")}
    return w, g, GOLD[tag + "/users"], GOLD[tag + "/items"], GOLD[tag + "/labels"], tuple(int(v) for v in GOLD[tag + "/shape"])


@pytest.mark.parametrize("tag", TAGS)
def test_the_numpy_yardstick_equals_the_reference_in_fp64(tag):
    w, g, users, items, labels, shape = fixture(tag)
    assert dcn_shape(w) == (shape[0], shape[1], shape[2], bool(shape[3]))
    nograd = sorted(str(k) for k in GOLD[tag + "/nograd"])
    assert nograd == [f"cross_net.layers.{c}.bias" for c in range(shape[2])]      # the reference's own .grad is None for them
    loss, logits, grads = dcn_head_grad_host(w, users, items, labels, np.float64)
    assert abs(loss - float(GOLD[tag + "/loss"])) <= 1e-12 and np.abs(logits - GOLD[tag + "/logits"]).max() <= 1e-12
    assert np.abs(dcn_head_host(w, users, items, np.float64) - GOLD[tag + "/logits"]).max() <= 1e-12
    assert sorted(grads) == sorted(g) == sorted(k for k in w if k not in nograd)
    degenerate = degenerate_keys(shape)
    largest = max(np.abs(g[k]).max() for k in g if k not in degenerate)
    for k in g:
        assert grads[k].shape == g[k].shape, k
        assert np.abs(grads[k] - g[k]).max() <= 1e-12 * (largest if k in degenerate else 1.0), k
    for k in degenerate:
        assert np.abs(g[k]).max() < 1e-6 * largest, k       # (what makes them degenerate, in the reference's own numbers)
    for key, ids in (("user_embeddings.weight", users), ("item_embeddings.weight", items)):
        untouched = np.setdiff1d(np.arange(len(w[key])), ids)
        assert len(untouched) == 1 and not grads[key][untouched].any()


@pytest.mark.parametrize("tag", TAGS)
def test_the_module_loads_the_reference_state_dict_strictly_and_gives_its_logits(tag):
    w, g, users, items, labels, (factor, deep, cross, ln) = fixture(tag)
    model = DCN(5, 7, factor_num=factor, deep_net_num_layers=deep, cross_net_num_layers=cross, use_layer_norm=bool(ln), layer_norm_eps=1e-12).double()
    assert sorted(model.state_dict()) == sorted(w)
    assert all(tuple(v.shape) == w[k].shape for k, v in model.state_dict().items())
    model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    logits = model((torch.from_numpy(users), torch.from_numpy(items)))
    assert np.abs(logits.detach().numpy() - GOLD[tag + "/logits"]).max() <= 1e-12
    torch.nn.functional.binary_cross_entropy_with_logits(logits, torch.from_numpy(labels).double()).backward()
    assert all(getattr(model.cross_net.layers, str(c)).bias.grad is None for c in range(cross))
    assert np.abs(model.item_embeddings.weight.grad.numpy() - g["item_embeddings.weight"]).max() <= 1e-12


def test_the_module_has_the_reference_constructor_and_initialisation():
    torch.manual_seed(3)
    model = DCN(11, 13, 8, 2, 3, 0.0, 0.0, True, 1e-12)
    sd = model.state_dict()
    assert sd["user_embeddings.weight"].shape == (11, 32) and sd["item_embeddings.weight"].shape == (13, 32)
    assert sd["deep_net.layers.0.linear.weight"].shape == (32, 64) and sd["deep_net.layers.1.linear.weight"].shape == (16, 32)
    assert sd["cross_net.layers.2.weight"].shape == (64, 1) and sd["cross_net.layers.2.bias"].shape == (64,)
    assert sd["output_layer.weight"].shape == (1, 64 + 16) and sd["output_layer.bias"].shape == (1,)
    assert float(sd["cross_net.layers.0.weight"].abs().max()) <= 1.0 < 1.2 * float(sd["cross_net.layers.0.weight"].abs().max())      # U(-1, 1)
    assert (sd["cross_net.layers.0.layer_norm.weight"] == 1).all() and (sd["deep_net.layers.1.layer_norm.bias"] == 0).all()
    assert 0.7 < float(sd["user_embeddings.weight"].std()) < 1.3      # N(0, 1)
    assert not any("layer_norm" in k for k in DCN(3, 3, 8, 1, 1).state_dict())


@pytest.mark.parametrize("tag", TAGS)
def test_the_decay_mask_is_the_decayed_group_of_the_reference_optimizer(tag):
    w, g, *_ = fixture(tag)
    decayed = sorted(str(k) for k in GOLD[tag + "/decayed"])
    assert sorted(k for k in w if decays(k)) == decayed
    assert any(k.endswith("layer_norm.weight") for k in decayed) == (tag != "noln")      # named layer_norm, not LayerNorm: they DO decay
    assert not any("bias" in k for k in decayed)


@pytest.mark.parametrize("shape", [(8, 1, 1, False), (8, 2, 3, True), (32, 3, 3, True), (64, 2, 6, True), (16, 4, 2, False)])
def test_layout(shape):
    factor, deep, cross, ln = shape
    layout, count = dcn_layout(*shape, 5, 7)
    E, D = factor << deep, 2 * (factor << deep)
    keys = list(layout)
    assert keys[:2] == ["user_embeddings.weight", "item_embeddings.weight"] and keys[-2:] == ["output_layer.weight", "output_layer.bias"]
    assert layout["user_embeddings.weight"] == (0, (5, E)) and layout["item_embeddings.weight"] == (5 * E, (7, E))
    at = 0
    for k, (off, shp) in layout.items():                     # packed in order, every offset a multiple of 8 floats
        assert off == at and off % 8 == 0, k
        at += int(np.prod(shp))
    assert at == count and layout["output_layer.bias"][1] == (1,) and layout["output_layer.weight"][1] == (1, D + 2 * factor)
    assert not any(re.fullmatch(r"cross_net\.layers\.\d+\.bias", k) for k in layout)
    assert any("layer_norm" in k for k in layout) == ln
    per_deep, per_cross = (4, 3) if ln else (2, 1)
    assert len(layout) == 2 + per_deep * deep + per_cross * cross + 2
    first_cross = keys.index("cross_net.layers.0.weight")
    assert all(k.startswith("deep_net") for k in keys[2:first_cross]) and all(k.startswith("cross_net") for k in keys[first_cross:-2])
    assert layout[f"deep_net.layers.{deep - 1}.linear.weight"][1] == (2 * factor, 4 * factor)
    slots = dcn_layout_slots(layout)
    assert len(slots) == _lib.DCN_TENSORS == 38 == 2 + 4 * _lib.DCN_MAX_DEEP + 3 * _lib.DCN_MAX_CROSS + 2
    assert slots[0] == 0 and slots[1] == 5 * E and slots[36] == layout["output_layer.weight"][0] and slots[37] == count - 1
    assert slots[2] == layout["deep_net.layers.0.linear.weight"][0] and slots[3] == layout["deep_net.layers.0.linear.bias"][0]
    assert slots[4] == (layout["deep_net.layers.0.layer_norm.weight"][0] if ln else -1)
    assert slots[18] == layout["cross_net.layers.0.weight"][0] and slots[20] == (layout["cross_net.layers.0.layer_norm.bias"][0] if ln else -1)
    assert all(s == -1 for s in slots[2 + 4 * deep: 18]) and all(s == -1 for s in slots[18 + 3 * cross: 36])
    assert sum(s >= 0 for s in slots) == len(layout)


def test_the_mirrored_constants_equal_the_defines_of_the_header():
    text = open(os.path.join(ROOT, "include", "pmgt_capi.h")).read()
    defines = {name: int(value) for name, value in re.findall(r"^#define (PMGT_DCN_\w+) (\d+)$", text, re.M)}
    assert defines == {"PMGT_DCN_MAX_DEEP": _lib.DCN_MAX_DEEP, "PMGT_DCN_MAX_CROSS": _lib.DCN_MAX_CROSS, "PMGT_DCN_TENSORS": _lib.DCN_TENSORS,
                       "PMGT_DCN_MAX_PAIRS": _lib.DCN_MAX_PAIRS}
    for sym in ("pmgt_dcn_layout", "pmgt_dcn_workspace_bytes", "pmgt_dcn_forward", "pmgt_dcn_train_grad"):
        assert sym in _lib.HIP_SYMBOLS and sym + "(" in text, sym
    assert _lib.DcnHeadC.params.offset == 40 and _lib.DcnHeadC.user_num.offset == 24      # 6 x 4 bytes, 2 x int64, 2 pointers


def test_the_head_module_imports_without_a_gpu_library():
    code = "import pmgt_amd.dcn_head; assert 'libpmgt_hip' not in open('/proc/self/maps').read(); print('ok')"
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", out.stderr


def test_refusals():
    for args, what in (((12, 2, 3), "factor_num"), ((8, 0, 3), "deep_net_num_layers"), ((8, 5, 3), "deep_net_num_layers"),
                       ((64, 3, 3), "above 256"), ((32, 4, 1), "above 256"), ((8, 2, 0), "cross_net_num_layers"), ((8, 2, 7), "cross_net_num_layers")):
        with pytest.raises(ValueError, match=what):
            check_dcn_covered(*args)
        with pytest.raises(ValueError, match=what):
            dcn_layout(*args, True, 5, 7)
    for f, l in ((8, 4), (16, 4), (32, 3), (64, 2), (64, 1)):    # every shape of the reference's configs is covered
        for c in (1, 6):
            check_dcn_covered(f, l, c)
    with pytest.raises(ValueError, match="user_num"):
        dcn_layout(8, 2, 3, True, 0, 7)
    with pytest.raises(ValueError, match="item_num"):
        dcn_layout(8, 2, 3, True, 5, 2 ** 31)
    for kw in (dict(emb_dropout=0.1), dict(dropout=0.2)):
        with pytest.raises(ValueError, match="dropout is not covered"):
            check_dcn_dropout(**{**dict(emb_dropout=0.0, dropout=0.0), **kw})
    check_dcn_dropout(0.0, 0.0)
    ok = (np.zeros(3, np.int64), np.zeros(3, np.int64), np.zeros(3, np.float32))
    check_dcn_pairs(*ok, 5, 7)
    with pytest.raises(ValueError, match="users"):
        check_dcn_pairs(np.array([0, 5, 1]), ok[1], ok[2], 5, 7)
    with pytest.raises(ValueError, match="items"):
        check_dcn_pairs(ok[0], np.array([0, -1, 1]), ok[2], 5, 7)
    with pytest.raises(ValueError, match="n = 0"):
        check_dcn_pairs(ok[0][:0], ok[1][:0], ok[2][:0], 5, 7)
    with pytest.raises(ValueError, match="n = 65537"):
        check_dcn_pairs(np.zeros(65537, np.int64), np.zeros(65537, np.int64), np.zeros(65537, np.float32), 5, 7)
    check_dcn_pairs(np.zeros(65536, np.int64), np.zeros(65536, np.int64), np.zeros(65536, np.float32), 5, 7)
    with pytest.raises(ValueError, match="must be one"):
        check_dcn_pairs(ok[0], ok[1][:2], ok[2], 5, 7)
    w, *_ = fixture("ln")
    with pytest.raises(ValueError, match="users"):
        dcn_head_grad_host(w, np.array([5]), np.array([0]), np.array([1.0]))
    with pytest.raises(ValueError, match="items"):
        dcn_head_host(w, np.array([0]), np.array([7]))


class FakeDropout:
    p = 0.1


class FakeModel:
    """What DcnTrainer, evaluate_ctr and fit_dcn read of a dcn.DCN before they touch a device."""
    user_num, item_num, factor_num, deep_layers, cross_layers, use_layer_norm, layer_norm_eps, dropout_p = 5, 7, 8, 2, 3, True, 1e-12, 0.0
    emb_dropout = FakeDropout()


def test_a_model_with_dropout_is_refused_by_the_trainer_the_fit_and_the_evaluation():
    from pmgt_amd.dcn_train import DcnTrainer, evaluate_ctr, fit_dcn
    pairs = np.array([[0, 1], [1, 2]])
    for call in (lambda m: DcnTrainer(m), lambda m: evaluate_ctr(m, pairs[:, 0], pairs[:, 1], np.ones(2)),
                 lambda m: fit_dcn(m, pairs, pairs, batch_size=2, max_epochs=1)):
        with pytest.raises(ValueError, match="dropout is not covered"):
            call(FakeModel())
    real = DCN(5, 7, 8, 2, 3, emb_dropout=0.0, dropout=0.3)
    with pytest.raises(ValueError, match="dropout is not covered"):
        DcnTrainer(real)


def test_ng_sample_labels_the_validation_pairs_as_the_dataset_does():
    """DCNDataset(valid_data, num_ng=max_sample_items).ng_sample(): features = the positives then max_sample_items negatives per positive,
    gt = labels = ones then zeros; a negative is never one of the user's items."""
    rng = np.random.default_rng(4)
    pairs = np.unique(np.stack([rng.integers(0, 9, 40), rng.integers(0, 30, 40)], axis=1), axis=0)
    P, k = len(pairs), 5
    users, items, labels = ng_sample(pairs, 9, 30, num_ng=k, seed=11)
    assert labels.dtype == np.float32 and np.array_equal(labels, np.concatenate([np.ones(P, np.float32), np.zeros(k * P, np.float32)]))
    assert np.array_equal(users[:P], pairs[:, 0]) and np.array_equal(items[:P], pairs[:, 1])
    assert np.array_equal(users[P:], np.repeat(pairs[:, 0], k))
    seen = set(map(tuple, pairs.tolist()))
    assert not any((int(u), int(i)) in seen for u, i in zip(users[P:], items[P:]))
    again = ng_sample(pairs, 9, 30, num_ng=k, seed=11)
    assert all(np.array_equal(a, b) for a, b in zip((users, items, labels), again))
