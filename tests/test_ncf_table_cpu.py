"""The host side of the trainable item table, no GPU: ncf_head_grad_host(table_grad=True) against what the reference's own NCF gives in fp64
with embed_item_MLP as a trained parameter (tests/golden/ncf_table_grad.npz, written by tests/golden/make_ncf_table_golden.py), the default
that returns no table gradient, normalize_item_table against the recorded sklearn.preprocessing.normalize, and the layout of the flat
buffer that holds the head and the table."""
import os

import numpy as np
import pytest
import torch

from pmgt_amd import ncf_head_grad_host, normalize_item_table
from pmgt_amd.ncf_train import TABLE_KEY, head_layout, table_layout
from tests.test_recommend_cpu import random_head

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ncf_table_grad.npz")


@pytest.mark.parametrize("tag", ["neumf", "mlp"])
def test_the_table_gradient_is_the_references(tag):
    g = np.load(GOLD)
    w = {k[len(tag) + 3:]: g[k] for k in g.files if k.startswith(f"{tag}/w/")}
    want = {k[len(tag) + 3:]: g[k] for k in g.files if k.startswith(f"{tag}/g/")}
    table = w.pop(TABLE_KEY)
    assert table.shape == (7, 16) and table.dtype == np.float64 and len(g[f"{tag}/users"]) == 33
    assert ("gmf_item_embeddings.weight" in w) == (tag == "neumf")
    loss, logits, grads = ncf_head_grad_host(w, table, g[f"{tag}/users"], g[f"{tag}/items"], g[f"{tag}/labels"], np.float64, table_grad=True)
    rel = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)
    assert rel(loss, g[f"{tag}/loss"]) <= 1e-12 and rel(logits, g[f"{tag}/logits"]) <= 1e-12
    assert sorted(grads) == sorted(want) == sorted(list(w) + [TABLE_KEY])
    for k in want:
        assert grads[k].shape == want[k].shape and grads[k].dtype == np.float64 and np.abs(want[k]).max() > 0, k
        assert rel(grads[k], want[k]) <= 1e-12, k
    # item 6 never appears: its row is exactly zero, in the fixture and here; every other item appears
    assert 6 not in g[f"{tag}/items"] and not want[TABLE_KEY][6].any()
    assert (grads[TABLE_KEY][6].view(np.uint64) == 0).all() and grads[TABLE_KEY][:6].any(axis=1).all()


def test_without_the_keyword_nothing_changes():
    w, table = random_head(8, 2, "NeuMF-end", user_num=5, n_items=7, seed=3)
    rng = np.random.default_rng(1)
    users, items, labels = rng.integers(0, 4, size=20), rng.integers(0, 6, size=20), (rng.random(20) < 0.4).astype(np.float32)
    for dt in (np.float64, np.float32):
        loss0, z0, g0 = ncf_head_grad_host(w, table, users, items, labels, dt)
        loss1, z1, g1 = ncf_head_grad_host(w, table, users, items, labels, dt, table_grad=True)
        assert TABLE_KEY not in g0 and sorted(g0) == sorted(w) and sorted(g1) == sorted(list(w) + [TABLE_KEY])
        assert loss0 == loss1 and np.array_equal(z0, z1) and all(np.array_equal(g0[k], g1[k]) for k in g0)
        assert g1[TABLE_KEY].dtype == dt and g1[TABLE_KEY].shape == table.shape


def test_normalize_item_table_is_sklearns_normalize():
    g = np.load(GOLD)
    x, want = g["norm/in"], g["norm/out"]
    assert x.shape == (9, 16) and x.dtype == np.float32 and want.dtype == np.float32 and not x[4].any() and x[[0, 8]].any(axis=1).all()
    keep = x.copy()
    got = normalize_item_table(x)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(x, keep)                           # the input is left as it is
    assert (got[4].view(np.uint32) == 0).all()               # the zero row stays zero
    assert np.abs(np.linalg.norm(np.delete(got, 4, axis=0).astype(np.float64), axis=1) - 1).max() < 1e-6
    t = normalize_item_table(torch.from_numpy(x))
    assert isinstance(t, torch.Tensor) and t.dtype == torch.float32 and np.array_equal(t.numpy().view(np.uint32), want.view(np.uint32))
    assert normalize_item_table(x.astype(np.float64)).dtype == np.float64
    with pytest.raises(ValueError, match="matrix"):
        normalize_item_table(np.zeros(4, np.float32))


@pytest.mark.parametrize("factor,num_layers,kind", [(8, 1, "MLP"), (8, 2, "NeuMF-end"), (64, 3, "NeuMF-end"), (32, 4, "MLP")])
def test_the_table_follows_the_head_at_a_multiple_of_eight_floats(factor, num_layers, kind):
    user_num, item_num = 11, 23
    d = factor << (num_layers - 1)
    head, head_count = head_layout(factor, num_layers, kind, user_num, item_num)
    layout, count = table_layout(factor, num_layers, kind, user_num, item_num)
    assert list(layout) == list(head) + [TABLE_KEY] and all(layout[k] == head[k] for k in head)
    off, shape = layout[TABLE_KEY]
    assert shape == (item_num, d) and off % 8 == 0 and head_count <= off < head_count + 8 and count == off + item_num * d
    assert head_count % 8 == 1 and off - head_count == 7      # the head ends with one float: seven pad floats
    # every float of the buffer belongs to exactly one named view, the pad to none
    owner = np.zeros(count, dtype=np.int32)
    for key, (o, s) in layout.items():
        owner[o: o + int(np.prod(s))] += 1
    assert (owner[:head_count] == 1).all() and (owner[head_count:off] == 0).all() and (owner[off:] == 1).all()
