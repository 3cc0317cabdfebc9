"""What the head of a PMGT_NCF is (pmgt/pmgt_ncf/models.py:91-105), stated once for the scoring (recommend.py), the training (ncf_train.py) and
the ranking evaluation (evaluation.py): which heads the kernels cover, the flat parameter layout, the refusals of the ids and tables that the
kernels read unchecked, and the numpy references that every NCF kernel is judged against (ncf_head_host: users x catalogue;
ncf_head_grad_host: loss, logits and every gradient of a list of pairs, under the masks of ncf_dropout_masks when the head is trained with
dropout; ncf_head_rows_grad_host: the same on an item row per pair, with the gradient of those rows).  What the head shares with the other pair head, the DCN -- check_ids, check_pairs, head_weights, the dropout RNG (ncf_dropout_keep is
pair_train.dropout_keep) -- lives in pair_train.py and is re-exported here.  Pure numpy and the bindings module: importing this loads no GPU library."""
import numpy as np

from ._lib import NCF_FACTORS, NCF_KINDS, NCF_MAX_D, NCF_MAX_LAYERS, NCF_SITE_EMB, NCF_SITE_GMF, NCF_SITE_LAYER
from .pair_train import _fmix32, check_dropout_p, check_ids, check_pairs, dropout_keep as ncf_dropout_keep  # noqa: F401
from .pair_train import dropout_scale as ncf_dropout_scale, head_weights, per_layer

HEAD_PREFIXES = ("mlp_user_embeddings.", "mlp_layers.", "predict_layer.", "gmf_user_embeddings.", "gmf_item_embeddings.")
TABLE_KEY = "item_table"                         # the trained table's name in the layouts, the gradients and the checkpoints
LAYER_DROPOUTS = "{} layer dropouts for {} layers"       # per_layer's refusal of a list of another length


def head_shape(weights: dict):
    """(factor_num, num_layers, kind, d) of a head given as a state_dict-keyed mapping."""
    num_layers = 0
    while f"mlp_layers.{num_layers}.linear.weight" in weights:
        num_layers += 1
    if num_layers < 1:
        raise ValueError("the head has no mlp_layers.0.linear.weight")
    d = int(weights["mlp_user_embeddings.weight"].shape[1])
    kind = "NeuMF-end" if weights.get("gmf_user_embeddings.weight") is not None else "MLP"
    return d >> (num_layers - 1), num_layers, kind, d


def check_head_covered(factor_num: int, num_layers: int, kind: str) -> None:
    """ValueError naming the limit when the kernels (pmgt_ncf_score, pmgt_ncf_train_grad, pmgt_ncf_train_grad_table) do not cover the head."""
    if kind not in NCF_KINDS:
        raise ValueError(f"ncf head: model kind {kind!r}, covered: {', '.join(map(repr, NCF_KINDS))}")
    if factor_num not in NCF_FACTORS:
        raise ValueError(f"ncf head: factor_num = {factor_num}, covered: {NCF_FACTORS}")
    if not 1 <= num_layers <= NCF_MAX_LAYERS:
        raise ValueError(f"ncf head: num_layers = {num_layers} outside [1, {NCF_MAX_LAYERS}]")
    if factor_num << (num_layers - 1) > NCF_MAX_D:
        raise ValueError(f"ncf head: d = factor_num * 2^(num_layers - 1) = {factor_num << (num_layers - 1)} above {NCF_MAX_D}")


def head_state(model) -> dict:
    """The head's entries of a PMGT_NCF's state_dict (what head_layout names)."""
    return {k: v for k, v in model.state_dict().items() if k.startswith(HEAD_PREFIXES)}


def head_layout(factor_num: int, num_layers: int, kind: str, user_num: int, item_num: int):
    """The flat parameter layout of pmgt_ncf_train_grad (include/pmgt_capi.h): -> ({state_dict key: (offset in floats, shape)} in buffer
    order, parameter count).  The three embedding tables come first, then weight and bias per layer (layer 0 UNSPLIT, [d, 2 d]), then the
    predict layer; every tensor but the last (predict_layer.bias, one float) has a multiple of 8 floats, so every offset is 32-byte aligned."""
    check_head_covered(factor_num, num_layers, kind)
    if not (isinstance(user_num, (int, np.integer)) and isinstance(item_num, (int, np.integer)) and 1 <= user_num < 2 ** 31 - 1
            and 1 <= item_num < 2 ** 31 - 1):
        raise ValueError(f"ncf_train: user_num = {user_num!r} and item_num = {item_num!r} must be integers in [1, 2^31 - 2]")
    d = factor_num << (num_layers - 1)
    shapes = [("mlp_user_embeddings.weight", (int(user_num), d))]
    if kind == "NeuMF-end":
        shapes += [("gmf_user_embeddings.weight", (int(user_num), factor_num)), ("gmf_item_embeddings.weight", (int(item_num), factor_num))]
    for i in range(num_layers):
        out = d >> i
        shapes += [(f"mlp_layers.{i}.linear.weight", (out, 2 * out)), (f"mlp_layers.{i}.linear.bias", (out,))]
    shapes += [("predict_layer.weight", (1, factor_num * (2 if kind == "NeuMF-end" else 1))), ("predict_layer.bias", (1,))]
    layout, at = {}, 0
    for key, shape in shapes:
        layout[key] = (at, shape)
        at += int(np.prod(shape))
    return layout, at


def table_layout(factor_num: int, num_layers: int, kind: str, user_num: int, item_num: int):
    """The flat buffer of a trainer that trains the item table: head_layout followed by TABLE_KEY [item_num, d], its offset rounded up to a
    multiple of 8 floats (the head ends with the one float of predict_layer.bias; the table's rows stay 32-byte aligned)
    -> (layout, count of the whole buffer).  The pad floats between the head and the table belong to no named tensor."""
    layout, count = head_layout(factor_num, num_layers, kind, user_num, item_num)
    off = (count + 7) // 8 * 8
    d = factor_num << (num_layers - 1)
    layout[TABLE_KEY] = (off, (int(item_num), d))
    return layout, off + int(item_num) * d


def layout_slots(layout: dict):
    """The offsets of `layout` in the slot order of pmgt_ncf_train_layout (-1: the head has no such tensor)."""
    slots = ["mlp_user_embeddings.weight", "gmf_user_embeddings.weight", "gmf_item_embeddings.weight"]
    slots += [f"mlp_layers.{i}.linear.{p}" for i in range(NCF_MAX_LAYERS) for p in ("weight", "bias")] + ["predict_layer.weight", "predict_layer.bias"]
    return [layout[k][0] if k in layout else -1 for k in slots]


def check_item_table(table, item_num, d: int, device, who: str) -> None:
    """ValueError in the name of `who` unless `table` is an fp32 torch tensor [item_num, d] on `device` (None: any row count from 1 / any GPU)."""
    import torch
    ok = isinstance(table, torch.Tensor) and table.dtype == torch.float32 and table.dim() == 2 and table.shape[1] == d
    ok = ok and (table.shape[0] >= 1 if item_num is None else table.shape[0] == item_num)
    if not (ok and (table.is_cuda if device is None else table.device == device)):
        raise ValueError(f"{who}: the item table must be an fp32 tensor [{item_num or 'I >= 1'}, {d}] on {device or 'a GPU'}")


def mlp_stack(w: dict, x: np.ndarray, num_layers: int) -> list:
    """[x, h_1, .., h_L] with h_(i+1) = relu(h_i W_i^T + b_i): layer 0 on the UNSPLIT concatenation [user ; item], as the torch head states it."""
    hs = [x]
    for i in range(num_layers):
        hs.append(np.maximum(hs[-1] @ w[f"mlp_layers.{i}.linear.weight"].T + w[f"mlp_layers.{i}.linear.bias"], 0))
    return hs


def ncf_dropout_masks(seed: int, step: int, n: int, factor_num: int, num_layers: int, kind: str, p_emb: float, p_layer) -> dict:
    """The masks pmgt_ncf_train_grad_dropout draws for a call on `n` pairs -> {site name: (bool keep [n, cols], fp32 scale)}:
    "emb" [n, 2 d] (the user half first), "layer<l>" [n, d >> l] for every layer and, NeuMF-end, "gmf" [n, factor_num] at p_emb with a
    mask of its own.  p_layer: one p for every layer or a sequence of num_layers.  What ncf_head_grad_host(masks=...) applies."""
    check_head_covered(factor_num, num_layers, kind)
    p_layer = per_layer(p_layer, num_layers, LAYER_DROPOUTS, "ncf_train")
    d = factor_num << (num_layers - 1)
    masks = {"emb": (ncf_dropout_keep(seed, step, NCF_SITE_EMB, n, 2 * d, p_emb), ncf_dropout_scale(p_emb))}
    if kind == "NeuMF-end":
        masks["gmf"] = (ncf_dropout_keep(seed, step, NCF_SITE_GMF, n, factor_num, p_emb), ncf_dropout_scale(p_emb))
    for i in range(num_layers):
        masks[f"layer{i}"] = (ncf_dropout_keep(seed, step, NCF_SITE_LAYER + i, n, d >> i, p_layer[i]), ncf_dropout_scale(p_layer[i]))
    return masks


def ncf_head_host(weights: dict, users, table, dtype=np.float64) -> np.ndarray:
    """PMGT_NCF.head in eval mode on plain arrays, every user of `users` against every row of `table` [I, d] -> logits [len(users), I] in
    `dtype`.  `weights` is keyed like the model's state_dict ("mlp_user_embeddings.weight", "mlp_layers.<i>.linear.weight" / ".bias",
    "predict_layer.weight" / ".bias" and, for NeuMF-end, "gmf_user_embeddings.weight" / "gmf_item_embeddings.weight"); arrays or CPU
    tensors."""
    w = head_weights(weights, dtype)
    _, num_layers, kind, d = head_shape(w)
    users = np.asarray(users, dtype=np.int64)
    table = np.asarray(table).astype(dtype)
    n, n_items = len(users), len(table)
    out = np.empty((n, n_items), dtype=dtype)
    per = max(1, (1 << 22) // (n_items * 2 * d))             # users per chunk of pair rows: about 4 M elements of layer 0's input
    for lo in range(0, n, per):
        u = users[lo: lo + per]
        m = len(u)
        x = np.concatenate([np.repeat(w["mlp_user_embeddings.weight"][u], n_items, axis=0), np.tile(table, (m, 1))], axis=1)
        h = mlp_stack(w, x, num_layers)[-1]
        if kind == "NeuMF-end":
            gmf = np.repeat(w["gmf_user_embeddings.weight"][u], n_items, axis=0) * np.tile(w["gmf_item_embeddings.weight"][:n_items], (m, 1))
            h = np.concatenate([gmf, h], axis=1)
        out[lo: lo + m] = (h @ w["predict_layer.weight"].T + w["predict_layer.bias"]).reshape(m, n_items)
    return out


def _head_grad(w: dict, x_item: np.ndarray, users, items, y, dtype, m: dict):
    """The one statement of the trained head's mathematics, shared by ncf_head_grad_host (x_item = table[items]) and
    ncf_head_rows_grad_host (x_item given per pair): `w` in `dtype`, x_item [n, d] the item half of layer 0's input, m = {site: mask in
    `dtype`} -> (loss, logits, the head's gradients, d loss / d x0 [n, 2 d] per pair, under the emb mask)."""
    factor, num_layers, kind, d = head_shape(w)
    n = len(users)
    one = dtype(1)
    x0 = np.concatenate([w["mlp_user_embeddings.weight"][users], x_item], axis=1)
    if not m:
        hs = mlp_stack(w, x0, num_layers)
    else:
        hs = [x0 * m["emb"] if "emb" in m else x0]
        for i in range(num_layers):
            a = hs[-1] @ w[f"mlp_layers.{i}.linear.weight"].T + w[f"mlp_layers.{i}.linear.bias"]
            hs.append(np.maximum(a * m[f"layer{i}"] if f"layer{i}" in m else a, 0))
    feat = hs[-1]
    if kind == "NeuMF-end":
        gu, gi = w["gmf_user_embeddings.weight"][users], w["gmf_item_embeddings.weight"][items]
        feat = np.concatenate([gu * gi * m["gmf"] if "gmf" in m else gu * gi, feat], axis=1)
    wp = w["predict_layer.weight"].reshape(-1)
    z = feat @ wp + w["predict_layer.bias"][0]               # (a matrix-vector product; ncf_head_host's is matrix-matrix: kept apart)
    e = np.exp(-np.abs(z))
    loss = (np.maximum(z, 0) - z * y + np.log1p(e)).sum(dtype=dtype) / dtype(n)
    dl = (np.where(z >= 0, one / (one + e), e / (one + e)) - y) / dtype(n)
    grads = {"predict_layer.weight": (dl @ feat).reshape(1, -1), "predict_layer.bias": dl.sum(dtype=dtype).reshape(1)}
    dfeat = dl[:, None] * wp[None, :]
    if kind == "NeuMF-end":
        dg, dh = dfeat[:, :factor], dfeat[:, factor:]
        if "gmf" in m:
            dg = dg * m["gmf"]
        grads["gmf_user_embeddings.weight"] = np.zeros_like(w["gmf_user_embeddings.weight"])
        grads["gmf_item_embeddings.weight"] = np.zeros_like(w["gmf_item_embeddings.weight"])
        np.add.at(grads["gmf_user_embeddings.weight"], users, dg * gi)
        np.add.at(grads["gmf_item_embeddings.weight"], items, dg * gu)
    else:
        dh = dfeat
    for i in reversed(range(num_layers)):
        dz = dh * m[f"layer{i}"] * (hs[i + 1] > 0) if f"layer{i}" in m else dh * (hs[i + 1] > 0)
        grads[f"mlp_layers.{i}.linear.weight"] = dz.T @ hs[i]
        grads[f"mlp_layers.{i}.linear.bias"] = dz.sum(axis=0, dtype=dtype)
        dh = dz @ w[f"mlp_layers.{i}.linear.weight"]
    if "emb" in m:
        dh = dh * m["emb"]
    grads["mlp_user_embeddings.weight"] = np.zeros_like(w["mlp_user_embeddings.weight"])
    np.add.at(grads["mlp_user_embeddings.weight"], users, dh[:, :d])
    assert all(g.dtype == dtype for g in grads.values()) and z.dtype == dtype and dh.dtype == dtype
    return dtype(loss), z, grads, dh


def _masks_as(masks, dtype) -> dict:
    return {} if masks is None else {k: np.asarray(keep, dtype=bool).astype(dtype) * dtype(scale) for k, (keep, scale) in masks.items()}


def ncf_head_grad_host(weights: dict, table, users, items, labels, dtype=np.float64, table_grad: bool = False, masks: dict = None):
    """PMGT_NCF.head with dropout 0 on the pairs (users[p], items[p]) over the frozen `table` [I, d], the mean BCE-with-logits loss against
    `labels` and its gradient, every operation in `dtype` -> (loss, logits [n], {state_dict key: gradient}).  `weights` is keyed like the
    model's state_dict (see ncf_head_host).  The loss is max(z, 0) - z y + log1p(exp(-|z|)), dlogit = (sigmoid(z) - y) / n with the sigmoid
    in its overflow-free form, the ReLU passes where h > 0, and rows of the embedding tables hit by several pairs are summed in pair order.
    table_grad=True: the gradients also hold TABLE_KEY ("item_table"), d loss / d table [I, d], by the same rule.
    masks: None, or {site: (bool keep [n, cols], scale)} as ncf_dropout_masks names them -- the head in TRAINING mode under these masks,
    m = keep * scale in `dtype`: x0 = m_emb [user ; item], h_(l+1) = relu(m_l (W_l h_l + b_l)), gmf = m_gmf (gmf_u gmf_i), and the
    gradients of that function (d x0 carries m_emb to the embedding rows and the table).  A site that is missing is not dropped."""
    w = head_weights(weights, dtype)
    d = head_shape(w)[3]
    table = np.asarray(table).astype(dtype)
    users, items, y = check_pairs(users, items, labels, len(w["mlp_user_embeddings.weight"]), len(table), max_pairs=1 << 40)
    loss, z, grads, dh = _head_grad(w, table[items], users, items, y.astype(dtype), dtype, _masks_as(masks, dtype))
    if table_grad:
        grads[TABLE_KEY] = np.zeros_like(table)
        np.add.at(grads[TABLE_KEY], items, dh[:, d:])
        assert grads[TABLE_KEY].dtype == dtype
    return loss, z, grads


def ncf_head_rows_grad_host(weights: dict, x_item, users, items, labels, dtype=np.float64, masks: dict = None):
    """ncf_head_grad_host for a head whose item input is A ROW PER PAIR (pmgt_ncf_train_grad_rows: the CLS state of the pair's own context):
    layer 0 reads x_item[p] [n, d] where that function reads table[items[p]], the GMF branch (NeuMF-end) still reads
    gmf_item_embeddings[items[p]] -> (loss, logits [n], {state_dict key: gradient}, d_item [n, d]).  Row p of d_item is d loss / d x_item[p],
    under the emb mask when `masks` holds one; nothing is summed across pairs.  The same rules and the same code as ncf_head_grad_host: with
    x_item = table[items] the first three results are that function's, and d_item summed per item is its "item_table" gradient."""
    w = head_weights(weights, dtype)
    _, _, kind, d = head_shape(w)
    x_item = np.asarray(x_item).astype(dtype)
    item_num = len(w["gmf_item_embeddings.weight"]) if kind == "NeuMF-end" else 1 << 62      # (an MLP head reads no row by item id)
    users, items, y = check_pairs(users, items, labels, len(w["mlp_user_embeddings.weight"]), item_num, max_pairs=1 << 40)
    if x_item.shape != (len(users), d):
        raise ValueError(f"ncf_train: x_item {x_item.shape} must be [n, d] = [{len(users)}, {d}]")
    loss, z, grads, dh = _head_grad(w, x_item, users, items, y.astype(dtype), dtype, _masks_as(masks, dtype))
    return loss, z, grads, np.ascontiguousarray(dh[:, d:])
