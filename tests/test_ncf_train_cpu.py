"""The host side of pmgt_amd.ncf_train, no GPU: ng_sample against what the reference drew (tests/golden/ncf_ng_sample.npz, written by
tests/golden/make_ncf_train_golden.py), ncf_head_grad_host against torch autograd in fp64 on the head's formula written with torch CPU
modules, the flat parameter layout, and the refusals that come before any device work."""
import os

import numpy as np
import pytest
import torch

from pmgt_amd import ncf_head_grad_host, ng_sample
from pmgt_amd.ncf_train import check_pairs, head_layout, layout_slots
from tests.test_recommend_cpu import random_head

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ncf_ng_sample.npz")


@pytest.mark.parametrize("num_ng", [1, 4])
@pytest.mark.parametrize("chunk", [1, 7, 1024])
def test_ng_sample_draws_what_the_reference_draws(num_ng, chunk):
    g = np.load(GOLD)
    users, items, labels = ng_sample(g["pairs"], int(g["num_user"]), int(g["num_item"]), num_ng, int(g[f"seed_ng{num_ng}"]), chunk=chunk)
    assert users.dtype == np.int64 and items.dtype == np.int64 and labels.dtype == np.float32
    assert np.array_equal(users, g[f"users_ng{num_ng}"]) and np.array_equal(items, g[f"items_ng{num_ng}"])
    assert np.array_equal(labels, g[f"labels_ng{num_ng}"])
    n_pos = len(g["pairs"])
    assert np.array_equal(users[:n_pos], g["pairs"][:, 0]) and np.array_equal(items[:n_pos], g["pairs"][:, 1])      # positives first, in order
    held = set(map(tuple, g["pairs"].tolist()))
    assert not any((int(u), int(i)) in held for u, i in zip(users[n_pos:], items[n_pos:]))
    greedy = int(g["greedy_user"])
    assert (g["pairs"][:, 0] == greedy).sum() >= 0.9 * int(g["num_item"])      # the fixture does force redraws


def test_ng_sample_refusals():
    with pytest.raises(ValueError, match="outside"):
        ng_sample([(0, 5)], 1, 5, 1, 0)
    with pytest.raises(ValueError, match="every item"):
        ng_sample([(0, 0), (0, 1), (1, 0)], 2, 2, 1, 0)
    with pytest.raises(ValueError, match="at least one pair"):
        ng_sample(np.zeros((0, 2), np.int64), 2, 2, 1, 0)
    u, i, y = ng_sample([(0, 0), (1, 1)], 2, 2, 0, 0)       # num_ng = 0: the positives alone
    assert u.tolist() == [0, 1] and i.tolist() == [0, 1] and y.tolist() == [1.0, 1.0]


def torch_head_grads(w, factor, num_layers, kind, table, users, items, labels):
    """PMGT_NCF.head's formula (pmgt_amd/pmgt_ncf.py:83-95) on torch CPU modules in fp64, BCEWithLogitsLoss, autograd."""
    from pmgt_amd.pmgt_ncf import MLPLayer
    t = lambda a: torch.from_numpy(np.asarray(a)).double()
    layers = torch.nn.Sequential(*[MLPLayer(factor * 2 ** (num_layers - i), factor * 2 ** (num_layers - i) // 2, dropout=0.0)
                                   for i in range(num_layers)]).double()
    predict = torch.nn.Linear(factor * (2 if kind == "NeuMF-end" else 1), 1).double()
    mlp_user = torch.nn.Embedding.from_pretrained(t(w["mlp_user_embeddings.weight"]), freeze=False)
    named = {"mlp_user_embeddings.weight": mlp_user.weight, "predict_layer.weight": predict.weight, "predict_layer.bias": predict.bias}
    with torch.no_grad():
        for i in range(num_layers):
            layers[i].linear.weight.copy_(t(w[f"mlp_layers.{i}.linear.weight"]))
            layers[i].linear.bias.copy_(t(w[f"mlp_layers.{i}.linear.bias"]))
            named[f"mlp_layers.{i}.linear.weight"], named[f"mlp_layers.{i}.linear.bias"] = layers[i].linear.weight, layers[i].linear.bias
        predict.weight.copy_(t(w["predict_layer.weight"]))
        predict.bias.copy_(t(w["predict_layer.bias"]))
    u, it = torch.from_numpy(users), torch.from_numpy(items)
    out = layers(torch.cat([mlp_user(u), t(table)[it]], dim=-1))
    if kind == "NeuMF-end":
        gmf_user = torch.nn.Embedding.from_pretrained(t(w["gmf_user_embeddings.weight"]), freeze=False)
        gmf_item = torch.nn.Embedding.from_pretrained(t(w["gmf_item_embeddings.weight"]), freeze=False)
        named["gmf_user_embeddings.weight"], named["gmf_item_embeddings.weight"] = gmf_user.weight, gmf_item.weight
        out = torch.cat([gmf_user(u) * gmf_item(it), out], dim=-1)
    logits = predict(out).view(-1)
    loss = torch.nn.BCEWithLogitsLoss()(logits, torch.from_numpy(labels).double())
    loss.backward()
    return loss.item(), logits.detach().numpy(), {k: p.grad.numpy() for k, p in named.items()}


@pytest.mark.parametrize("factor,num_layers,kind", [(8, 1, "MLP"), (8, 1, "NeuMF-end"), (16, 2, "MLP"), (8, 2, "NeuMF-end"), (16, 3, "MLP"),
                                                    (32, 3, "NeuMF-end")])
def test_ncf_head_grad_host_is_autograd_on_the_heads_formula(factor, num_layers, kind):
    w, table = random_head(factor, num_layers, kind, user_num=5, n_items=7, seed=50 + factor + num_layers)
    rng = np.random.default_rng(factor * num_layers)
    n = 40                                                   # 40 pairs over 4 users x 6 items: every user and item comes several times
    users, items = rng.integers(0, 4, size=n), rng.integers(0, 6, size=n)
    labels = (rng.random(n) < 0.4).astype(np.float32)
    loss, logits, grads = ncf_head_grad_host(w, table, users, items, labels)
    t_loss, t_logits, t_grads = torch_head_grads(w, factor, num_layers, kind, table, users, items, labels)
    rel = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)
    assert loss.dtype == np.float64 and logits.dtype == np.float64 and logits.shape == (n,)
    assert rel(loss, t_loss) <= 1e-12 and rel(logits, t_logits) <= 1e-12
    assert sorted(grads) == sorted(t_grads) == sorted(w)
    for k in w:
        assert grads[k].shape == w[k].shape and grads[k].dtype == np.float64
        assert rel(grads[k], t_grads[k]) <= 1e-12, k
    # user 4 and item 6 never appear: their rows are exactly zero
    assert not grads["mlp_user_embeddings.weight"][4].any() and grads["mlp_user_embeddings.weight"][:4].any(axis=1).all()
    if kind == "NeuMF-end":
        assert not grads["gmf_user_embeddings.weight"][4].any() and not grads["gmf_item_embeddings.weight"][6].any()
    l32, z32, g32 = ncf_head_grad_host(w, table, users, items, labels, np.float32)
    assert l32.dtype == np.float32 and z32.dtype == np.float32 and all(g.dtype == np.float32 for g in g32.values())
    assert rel(z32, logits) < 1e-4


def test_saturated_logits_stay_finite_on_the_host():
    w, table = random_head(8, 2, "NeuMF-end", user_num=5, n_items=7, seed=3)
    users, items = np.array([0, 1, 2, 3]), np.array([0, 1, 2, 3])
    _, z, _ = ncf_head_grad_host(w, table, users, items, np.zeros(4, np.float32))
    w["predict_layer.weight"] = w["predict_layer.weight"] * np.float32(400.0 / np.abs(z - w["predict_layer.bias"][0]).min())
    _, z, _ = ncf_head_grad_host(w, table, users, items, np.zeros(4, np.float32))
    labels = (z < 0).astype(np.float32)                      # every label on the wrong side
    for dt in (np.float64, np.float32):
        loss, z, grads = ncf_head_grad_host(w, table, users, items, labels, dt)
        assert np.abs(z).min() > 100 and np.isfinite(loss) and loss > 100 and all(np.isfinite(g).all() for g in grads.values())


@pytest.mark.parametrize("factor,num_layers,kind", [(8, 1, "MLP"), (64, 2, "NeuMF-end"), (32, 4, "MLP"), (64, 3, "NeuMF-end")])
def test_layout_round_trip(factor, num_layers, kind):
    user_num, item_num = 11, 23
    layout, count = head_layout(factor, num_layers, kind, user_num, item_num)
    w, _ = random_head(factor, num_layers, kind, user_num, item_num, seed=1)
    assert list(layout) == [k for k in layout if k in w] and sorted(layout) == sorted(w)
    flat = np.full(count, np.nan, dtype=np.float32)
    at = 0
    for key, (off, shape) in layout.items():                 # packed in order, no gap, no overlap
        assert off == at and tuple(shape) == w[key].shape and (off % 8 == 0)
        flat[off: off + w[key].size] = w[key].reshape(-1)
        at += w[key].size
    assert at == count and not np.isnan(flat).any()
    for key, (off, shape) in layout.items():
        assert np.array_equal(flat[off: off + int(np.prod(shape))].reshape(shape), w[key])
    slots = layout_slots(layout)
    assert len(slots) == 13 and slots[0] == 0 and slots[12] == count - 1
    assert (slots[1] == -1) == (kind == "MLP") and [s for s in slots if s >= 0] == sorted(s for s in slots if s >= 0)
    assert all((slots[3 + 2 * i] >= 0) == (i < num_layers) for i in range(4))
    # the embedding tables come first: one contiguous region that the kernels zero
    assert layout["mlp_layers.0.linear.weight"][0] == user_num * (factor << (num_layers - 1)) + (0 if kind == "MLP" else (user_num + item_num) * factor)


def test_refusals_that_need_no_device():
    for bad, what in (((4, 2, "MLP"), "factor_num"), ((8, 5, "MLP"), "num_layers"), ((64, 4, "MLP"), "above 256"), ((8, 2, "GMF"), "kind")):
        with pytest.raises(ValueError, match=what):
            head_layout(*bad, 3, 4)
    with pytest.raises(ValueError, match="user_num"):
        head_layout(8, 2, "MLP", 0, 4)
    ok = (np.array([0, 1]), np.array([2, 3]), np.array([0.0, 1.0]))
    assert check_pairs(*ok, 2, 4)[2].dtype == np.float32
    for args, what in (((np.array([0, 2]), ok[1], ok[2], 2, 4), "users"), ((np.array([-1, 0]), ok[1], ok[2], 2, 4), "users"),
                       ((ok[0], np.array([0, 4]), ok[2], 2, 4), "items"), ((ok[0], ok[1], np.zeros(3), 2, 4), r"one \[n\]"),
                       ((np.zeros(0), np.zeros(0), np.zeros(0), 2, 4), "n = 0"), ((ok[0], ok[1], ok[2], 2, 4, 1), "n = 2")):
        with pytest.raises(ValueError, match=what):
            check_pairs(*args)
    w, table = random_head(8, 2, "MLP", 3, 4, seed=1)
    with pytest.raises(ValueError, match="items"):
        ncf_head_grad_host(w, table, [0], [4], [1.0])
