"""The host side of the NCF head's dropout, no GPU: ncf_dropout_keep (the counter-based hash restated in product code) against
tests/dropout_util.keep (the restatement the encoder's dropout tests trust), ncf_head_grad_host(masks=...) in fp64 against fp64 torch
autograd through the project's own PMGT_NCF.head with every Dropout module replaced by a stub that multiplies by the given keep * scale,
masks=None against the function as it was, and the refusals that need no device."""
import re
import types

import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.ncf_head import TABLE_KEY, mlp_stack, ncf_dropout_keep, ncf_dropout_masks, ncf_dropout_scale, ncf_head_grad_host
from tests import dropout_util as du
from tests.test_recommend_cpu import random_head


def ncf_sites(num_layers=4):
    return [_lib.NCF_SITE_EMB, _lib.NCF_SITE_GMF] + [_lib.NCF_SITE_LAYER + i for i in range(num_layers)]


def test_the_site_ids_are_distinct_and_the_headers():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    assert len(set(ncf_sites())) == 6
    hdr = open(os.path.join(root, "include", "pmgt_capi.h")).read()
    dev = open(os.path.join(root, "pmgt_amd", "ops", "ncf_head.h")).read()
    assert f"NCF_SITE_EMB = {_lib.NCF_SITE_EMB}, NCF_SITE_GMF = {_lib.NCF_SITE_GMF}, NCF_SITE_LAYER = {_lib.NCF_SITE_LAYER};" in dev
    for name, value in (("EMB", _lib.NCF_SITE_EMB), ("GMF", _lib.NCF_SITE_GMF), ("LAYER", _lib.NCF_SITE_LAYER)):
        assert re.search(rf"NCF_SITE_{name} +{value}\b", hdr), name      # documented with the entry
    assert "pmgt_ncf_train_grad_dropout(" in hdr and "pmgt_ncf_train_grad_dropout" in _lib.HIP_SYMBOLS


@pytest.mark.parametrize("p", [0.1, 0.5, 0.8])
@pytest.mark.parametrize("cols", [8, 30, 512])
def test_ncf_dropout_keep_is_the_hash_of_the_kernels(p, cols):
    rows = 130
    for site in ncf_sites():
        for seed, step in ((0, 0), (1234567, 7), (-5, 2 ** 33 + 1), (2 ** 62 + 99, 19)):
            got = ncf_dropout_keep(seed, step, site, rows, cols, p)
            assert got.dtype == bool and got.shape == (rows, cols)
            assert np.array_equal(got, du.keep(seed, step, site, rows, cols, p)), (site, seed, step)
    assert abs(got.mean() - (1 - p)) < 0.02 or cols == 8      # (130 x 8: too few draws for that)
    assert ncf_dropout_keep(3, 4, _lib.NCF_SITE_EMB, rows, cols, 0.0).all()
    assert ncf_dropout_scale(p) == np.float32(du.drop_scale(p)) and ncf_dropout_scale(p).dtype == np.float32


def test_ncf_dropout_masks_names_shapes_and_sites():
    m = ncf_dropout_masks(11, 3, 33, 16, 3, "NeuMF-end", 0.5, [0.1, 0.0, 0.8])
    assert list(m) == ["emb", "gmf", "layer0", "layer1", "layer2"]
    assert [m[k][0].shape for k in m] == [(33, 128), (33, 16), (33, 64), (33, 32), (33, 16)]
    assert np.array_equal(m["emb"][0], du.keep(11, 3, _lib.NCF_SITE_EMB, 33, 128, 0.5))
    assert np.array_equal(m["gmf"][0], du.keep(11, 3, _lib.NCF_SITE_GMF, 33, 16, 0.5))
    assert not np.array_equal(m["gmf"][0], m["emb"][0][:, :16])      # a mask of its own
    assert np.array_equal(m["layer2"][0], du.keep(11, 3, _lib.NCF_SITE_LAYER + 2, 33, 16, 0.8))
    assert m["layer1"][0].all() and m["layer1"][1] == 1.0 and m["emb"][1] == np.float32(2.0) and m["layer0"][1] == np.float32(du.drop_scale(0.1))
    assert list(ncf_dropout_masks(11, 3, 5, 8, 1, "MLP", 0.2, 0.3)) == ["emb", "layer0"]
    assert not np.array_equal(m["emb"][0], ncf_dropout_masks(11, 4, 33, 16, 3, "NeuMF-end", 0.5, 0.0)["emb"][0])      # the step drives them


class MaskStub(torch.nn.Module):
    """Stands in for an nn.Dropout: multiplies its input by the next of the given masks (keep * scale), in call order."""

    def __init__(self, *masks):
        super().__init__()
        self.masks, self.calls = [torch.from_numpy(np.asarray(k, dtype=np.float64) * np.float64(s)) for k, s in masks], 0

    def forward(self, x):
        m = self.masks[self.calls]
        self.calls += 1
        assert m.shape == x.shape
        return x * m


def torch_head_grads_with_masks(w, factor, num_layers, kind, table, users, items, labels, masks):
    """fp64 autograd through PMGT_NCF.head itself (pmgt_amd/pmgt_ncf.py:83-95) on a stand-in for `self` that holds the head's modules on
    the CPU (the class's constructor builds the encoder's engine, which needs the device)."""
    from pmgt_amd.pmgt_ncf import PMGT_NCF, MLPLayer
    t = lambda a: torch.from_numpy(np.asarray(a)).double()
    me = types.SimpleNamespace(model=kind)
    me.mlp_user_embeddings = torch.nn.Embedding.from_pretrained(t(w["mlp_user_embeddings.weight"]), freeze=False)
    me.emb_dropout = MaskStub(masks["emb"], *([masks["gmf"]] if kind == "NeuMF-end" else []))      # interaction first, then gmf
    me.mlp_layers = torch.nn.Sequential(*[MLPLayer(factor * 2 ** (num_layers - i), factor * 2 ** (num_layers - i) // 2, dropout=0.5)
                                          for i in range(num_layers)]).double()
    me.predict_layer = torch.nn.Linear(factor * (2 if kind == "NeuMF-end" else 1), 1).double()
    named = {"mlp_user_embeddings.weight": me.mlp_user_embeddings.weight, "predict_layer.weight": me.predict_layer.weight,
             "predict_layer.bias": me.predict_layer.bias}
    with torch.no_grad():
        for i in range(num_layers):
            lin = me.mlp_layers[i].linear
            lin.weight.copy_(t(w[f"mlp_layers.{i}.linear.weight"]))
            lin.bias.copy_(t(w[f"mlp_layers.{i}.linear.bias"]))
            named[f"mlp_layers.{i}.linear.weight"], named[f"mlp_layers.{i}.linear.bias"] = lin.weight, lin.bias
            me.mlp_layers[i].dropout = MaskStub(masks[f"layer{i}"])
        me.predict_layer.weight.copy_(t(w["predict_layer.weight"]))
        me.predict_layer.bias.copy_(t(w["predict_layer.bias"]))
    if kind == "NeuMF-end":
        me.gmf_user_embeddings = torch.nn.Embedding.from_pretrained(t(w["gmf_user_embeddings.weight"]), freeze=False)
        me.gmf_item_embeddings = torch.nn.Embedding.from_pretrained(t(w["gmf_item_embeddings.weight"]), freeze=False)
        named["gmf_user_embeddings.weight"], named["gmf_item_embeddings.weight"] = me.gmf_user_embeddings.weight, me.gmf_item_embeddings.weight
    tab = t(table).requires_grad_(True)
    named[TABLE_KEY] = tab
    u, it = torch.from_numpy(users), torch.from_numpy(items)
    logits = PMGT_NCF.head(me, u, it, tab[it])
    loss = torch.nn.BCEWithLogitsLoss()(logits, torch.from_numpy(labels).double())
    loss.backward()
    assert me.emb_dropout.calls == len(me.emb_dropout.masks) and all(layer.dropout.calls == 1 for layer in me.mlp_layers)
    return loss.item(), logits.detach().numpy(), {k: p.grad.numpy() for k, p in named.items()}


@pytest.mark.parametrize("factor,num_layers,kind", [(8, 1, "MLP"), (16, 3, "NeuMF-end"), (32, 2, "NeuMF-end")])
@pytest.mark.parametrize("p_emb,p_layer", [(0.5, 0.0), (0.0, 0.5), (0.2, [0.3, 0.1, 0.6])])
def test_the_masked_host_gradient_is_autograd_through_the_heads_own_formula(factor, num_layers, kind, p_emb, p_layer):
    w, table = random_head(factor, num_layers, kind, user_num=5, n_items=7, seed=70 + factor + num_layers)
    rng = np.random.default_rng(factor * num_layers)
    n = 33
    users, items = rng.integers(0, 4, size=n), rng.integers(0, 6, size=n)
    labels = (rng.random(n) < 0.4).astype(np.float32)
    p_layer = p_layer[:num_layers] if isinstance(p_layer, list) else p_layer
    masks = ncf_dropout_masks(97, 5, n, factor, num_layers, kind, p_emb, p_layer)
    loss, logits, grads = ncf_head_grad_host(w, table, users, items, labels, table_grad=True, masks=masks)
    t_loss, t_logits, t_grads = torch_head_grads_with_masks(w, factor, num_layers, kind, table, users, items, labels, masks)
    rel = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)
    assert loss.dtype == np.float64 and logits.dtype == np.float64
    assert rel(loss, t_loss) <= 1e-12 and rel(logits, t_logits) <= 1e-12
    assert sorted(grads) == sorted(t_grads) == sorted(list(w) + [TABLE_KEY])
    for k in grads:
        assert grads[k].dtype == np.float64 and grads[k].shape == t_grads[k].shape and rel(grads[k], t_grads[k]) <= 1e-12, k
    # the masks do something: the logits differ from the head without dropout
    assert rel(logits, ncf_head_grad_host(w, table, users, items, labels)[1]) > 1e-3
    l32, z32, g32 = ncf_head_grad_host(w, table, users, items, labels, np.float32, table_grad=True, masks=masks)
    assert l32.dtype == np.float32 and z32.dtype == np.float32 and all(g.dtype == np.float32 for g in g32.values())
    assert rel(z32, logits) < 1e-4


def grad_host_as_it_was(weights, table, users, items, labels, dtype, table_grad):
    """ncf_head_grad_host before it took masks, line for line (numpy only)."""
    from pmgt_amd.ncf_head import check_pairs, head_shape, head_weights
    w = head_weights(weights, dtype)
    factor, num_layers, kind, d = head_shape(w)
    table = np.asarray(table).astype(dtype)
    users, items, y = check_pairs(users, items, labels, len(w["mlp_user_embeddings.weight"]), len(table), max_pairs=1 << 40)
    y = y.astype(dtype)
    n = len(users)
    one = dtype(1)
    hs = mlp_stack(w, np.concatenate([w["mlp_user_embeddings.weight"][users], table[items]], axis=1), num_layers)
    feat = hs[-1]
    if kind == "NeuMF-end":
        gu, gi = w["gmf_user_embeddings.weight"][users], w["gmf_item_embeddings.weight"][items]
        feat = np.concatenate([gu * gi, feat], axis=1)
    wp = w["predict_layer.weight"].reshape(-1)
    z = feat @ wp + w["predict_layer.bias"][0]
    e = np.exp(-np.abs(z))
    loss = (np.maximum(z, 0) - z * y + np.log1p(e)).sum(dtype=dtype) / dtype(n)
    dl = (np.where(z >= 0, one / (one + e), e / (one + e)) - y) / dtype(n)
    grads = {"predict_layer.weight": (dl @ feat).reshape(1, -1), "predict_layer.bias": dl.sum(dtype=dtype).reshape(1)}
    dfeat = dl[:, None] * wp[None, :]
    if kind == "NeuMF-end":
        dg, dh = dfeat[:, :factor], dfeat[:, factor:]
        grads["gmf_user_embeddings.weight"] = np.zeros_like(w["gmf_user_embeddings.weight"])
        grads["gmf_item_embeddings.weight"] = np.zeros_like(w["gmf_item_embeddings.weight"])
        np.add.at(grads["gmf_user_embeddings.weight"], users, dg * gi)
        np.add.at(grads["gmf_item_embeddings.weight"], items, dg * gu)
    else:
        dh = dfeat
    for i in reversed(range(num_layers)):
        dz = dh * (hs[i + 1] > 0)
        grads[f"mlp_layers.{i}.linear.weight"] = dz.T @ hs[i]
        grads[f"mlp_layers.{i}.linear.bias"] = dz.sum(axis=0, dtype=dtype)
        dh = dz @ w[f"mlp_layers.{i}.linear.weight"]
    grads["mlp_user_embeddings.weight"] = np.zeros_like(w["mlp_user_embeddings.weight"])
    np.add.at(grads["mlp_user_embeddings.weight"], users, dh[:, :d])
    if table_grad:
        grads[TABLE_KEY] = np.zeros_like(table)
        np.add.at(grads[TABLE_KEY], items, dh[:, d:])
    return dtype(loss), z, grads


@pytest.mark.parametrize("factor,num_layers,kind", [(8, 1, "MLP"), (8, 2, "NeuMF-end"), (16, 3, "MLP"), (64, 2, "NeuMF-end")])
def test_without_masks_the_host_gradient_has_the_bits_it_had(factor, num_layers, kind):
    w, table = random_head(factor, num_layers, kind, user_num=5, n_items=7, seed=9 + factor)
    rng = np.random.default_rng(3)
    users, items = rng.integers(0, 4, size=40), rng.integers(0, 6, size=40)
    labels = (rng.random(40) < 0.4).astype(np.float32)
    for dtype in (np.float64, np.float32):
        for tg in (False, True):
            new, old = ncf_head_grad_host(w, table, users, items, labels, dtype, table_grad=tg), grad_host_as_it_was(w, table, users, items, labels, dtype, tg)
            assert new[0].tobytes() == old[0].tobytes() and new[1].tobytes() == old[1].tobytes() and sorted(new[2]) == sorted(old[2])
            assert all(new[2][k].tobytes() == old[2][k].tobytes() for k in old[2])
            # every p = 0: masks of ones and scale 1 change no bit either
            ones = ncf_head_grad_host(w, table, users, items, labels, dtype, table_grad=tg,
                                      masks=ncf_dropout_masks(1, 2, 40, factor, num_layers, kind, 0.0, 0.0))
            assert ones[1].tobytes() == old[1].tobytes() and all(ones[2][k].tobytes() == old[2][k].tobytes() for k in old[2])


def test_refusals_that_need_no_device():
    for bad in (1.0, 1.5, -0.1, float("nan")):
        with pytest.raises(ValueError, match=r"outside \[0, 1\)"):
            ncf_dropout_keep(0, 0, _lib.NCF_SITE_EMB, 4, 8, bad)
        with pytest.raises(ValueError, match=r"outside \[0, 1\)"):
            ncf_dropout_masks(0, 0, 4, 8, 2, "MLP", bad, 0.0)
        with pytest.raises(ValueError, match=r"outside \[0, 1\)"):
            ncf_dropout_masks(0, 0, 4, 8, 2, "MLP", 0.0, [0.1, bad])
    with pytest.raises(ValueError, match="layer dropouts"):
        ncf_dropout_masks(0, 0, 4, 8, 2, "MLP", 0.0, [0.1])
    with pytest.raises(ValueError, match="factor_num"):
        ncf_dropout_masks(0, 0, 4, 12, 2, "MLP", 0.0, 0.1)
