"""ncf_head_rows_grad_host, the yardstick of pmgt_ncf_train_grad_rows (the head on an item row PER PAIR), against ncf_head_grad_host: with
x_item = table[items] the two run the same code, so loss, logits and every head gradient are equal EXACTLY, and the per-pair rows of d_item
summed per item are the table's gradient (to fp64 rounding: np.add.at adds the same rows in the same order, so in fact exactly).  No GPU."""
import numpy as np
import pytest

from pmgt_amd.ncf_head import TABLE_KEY, ncf_dropout_masks, ncf_head_grad_host, ncf_head_rows_grad_host
from tests.test_recommend_cpu import random_head

HEADS = [(8, 1, "MLP"), (32, 3, "NeuMF-end")]
USER_NUM, ITEM_NUM, N = 6, 9, 47


def case(shape, seed=3):
    w, table = random_head(*shape, USER_NUM, ITEM_NUM, seed=100 + shape[0])
    rng = np.random.default_rng(seed)
    users, items = rng.integers(0, USER_NUM - 1, size=N), rng.integers(0, ITEM_NUM - 1, size=N)      # duplicates are forced: 47 pairs, 5 x 8 ids
    users[:3], items[:3] = (0, 1, 0), (2, 2, 2)              # item 2 under two users, and one exact duplicate pair
    labels = (rng.random(N) < 0.4).astype(np.float32)
    return w, table, users, items, labels


@pytest.mark.parametrize("shape", HEADS, ids=lambda s: f"f{s[0]}-L{s[1]}-{s[2]}")
@pytest.mark.parametrize("dropout", [False, True], ids=["plain", "p0.3"])
def test_rows_on_table_rows_is_the_table_function(shape, dropout):
    w, table, users, items, labels = case(shape)
    masks = ncf_dropout_masks(11, 5, N, *shape, 0.3, 0.3) if dropout else None
    loss, logits, grads = ncf_head_grad_host(w, table, users, items, labels, table_grad=True, masks=masks)
    r_loss, r_logits, r_grads, d_item = ncf_head_rows_grad_host(w, table[items], users, items, labels, masks=masks)
    assert r_loss == loss and r_loss.dtype == np.float64
    assert np.array_equal(r_logits, logits)
    assert set(r_grads) == set(grads) - {TABLE_KEY}
    for k, g in r_grads.items():
        assert np.array_equal(g, grads[k]), k
    assert d_item.shape == (N, table.shape[1]) and d_item.dtype == np.float64
    summed = np.zeros_like(grads[TABLE_KEY])
    np.add.at(summed, items, d_item)
    np.testing.assert_allclose(summed, grads[TABLE_KEY], rtol=1e-14, atol=1e-300)
    if dropout:                                              # d_item carries the emb mask: a dropped input element has no gradient
        keep = masks["emb"][0][:, table.shape[1]:]
        assert not keep.all() and not d_item[~keep].any() and d_item[keep].any()
    # two pairs on ONE item with different users keep different rows; the exact duplicate pair differs from the first only by its label
    assert items[0] == items[1] and users[0] != users[1] and not np.array_equal(d_item[0], d_item[1])


def test_rows_take_any_item_row_and_refuse_another_shape():
    shape = (8, 2, "NeuMF-end")
    w, table, users, items, labels = case(shape)
    rng = np.random.default_rng(9)
    x = rng.standard_normal((N, table.shape[1])).astype(np.float32)
    loss, logits, grads, d_item = ncf_head_rows_grad_host(w, x, users, items, labels)
    # central differences on two elements of x_item: d_item is the gradient of the loss with respect to THAT pair's row
    for p, c in ((0, 1), (5, 7)):
        h = 1e-6
        xp, xm = x.astype(np.float64), x.astype(np.float64)
        xp[p, c] += h
        xm[p, c] -= h
        num = (ncf_head_rows_grad_host(w, xp, users, items, labels)[0] - ncf_head_rows_grad_host(w, xm, users, items, labels)[0]) / (2 * h)
        assert abs(num - d_item[p, c]) <= 1e-8 + 1e-5 * abs(d_item[p, c])
    with pytest.raises(ValueError, match="x_item"):
        ncf_head_rows_grad_host(w, x[:-1], users, items, labels)
    with pytest.raises(ValueError, match="items"):
        ncf_head_rows_grad_host(w, x, users, items + ITEM_NUM, labels)      # (NeuMF-end: items address gmf_item_embeddings)


def test_rows_entry_is_declared_and_bound():
    import os
    from pmgt_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pmgt_capi.h")).read()
    for sym in ("pmgt_ncf_train_grad_rows", "pmgt_ncf_train_rows_workspace_bytes"):
        assert sym + "(" in hdr and sym in _lib.HIP_SYMBOLS
    ops = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pmgt_ops.h")).read()
    for sym in ("pmgt_op_adamw_segments", "pmgt_op_cls_gather", "pmgt_op_cls_scatter"):
        assert sym + "(" in ops and sym in _lib.OPS_SYMBOLS
