"""What the reference's stand-alone NCF model is (pmgt/ncf/models.py; the class is ncf.py), stated once for the training
(ncf_model_train.py) and its tests: which shapes the kernels cover, the flat parameter layout of pmgt_ncf_model_train_grad under the NCF
class's state_dict keys, and the numpy yardstick every kernel of ops/ncf_model_train.hip is judged against.  With d = F 2^(L - 1):
  h_0 = m_e [embed_user_MLP[u] ; embed_item_MLP[i]],   h_(l+1) = relu(LN_l(m_l (W_l h_l + b_l)))
  g   = m_g (embed_user_GMF[u] * embed_item_GMF[i])
  z   = predict_layer . h_L (MLP) | . g (GMF) | . [g ; h_L] (NeuMF-end, NeuMF-pre)  + predict_layer.bias,   loss = mean BCE-with-logits
LN is torch.nn.LayerNorm (biased variance), absent without use_layer_norm; the masks m = 0 or 1 / (1 - p) are ncf_dropout_masks' (the
dropout sits before the LayerNorm: dropped zeros enter its statistics).  Without LayerNorm, kinds MLP / NeuMF-end, this is the head of
ncf_head.py over a trained or frozen table, and the layout is table_layout's / head_layout's under the key map
  embed_user_MLP -> mlp_user_embeddings, embed_user_GMF / embed_item_GMF -> gmf_*, MLP_layers.{3i} -> mlp_layers.{i}.linear,
  embed_item_MLP.weight -> item_table.
Pure numpy and the bindings module: importing this loads no GPU library."""
import numpy as np

from ._lib import NCF_FACTORS, NCF_MAX_D, NCF_MAX_LAYERS, NCF_MODEL_KINDS, NCF_MODEL_TENSORS
from .dcn_head import _ln, _ln_bwd
from .ncf_head import _masks_as
from .pair_train import check_pairs, head_weights

USER_MLP, ITEM_MLP, USER_GMF, ITEM_GMF = "embed_user_MLP.weight", "embed_item_MLP.weight", "embed_user_GMF.weight", "embed_item_GMF.weight"
OUT_W, OUT_B = "predict_layer.weight", "predict_layer.bias"


def linear_key(i: int, use_layer_norm: bool) -> str:
    """The module of layer i's Linear in MLP_layers (Linear, Dropout, [LayerNorm,] ReLU per layer)."""
    return f"MLP_layers.{(4 if use_layer_norm else 3) * i}"


def norm_key(i: int) -> str:
    return f"MLP_layers.{4 * i + 2}"


def layer_keys(i: int, use_layer_norm: bool) -> list:
    """W, b[, gamma, beta] of layer i under the state_dict's keys."""
    p = linear_key(i, use_layer_norm)
    return [p + ".weight", p + ".bias"] + ([norm_key(i) + ".weight", norm_key(i) + ".bias"] if use_layer_norm else [])


def reads_mlp(kind: str) -> bool:
    return kind != "GMF"


def reads_gmf(kind: str) -> bool:
    return kind != "MLP"


def check_ncf_model_covered(factor_num: int, num_layers: int, kind: str, layer_norm_eps: float = 1e-12) -> None:
    """ValueError naming the limit when pmgt_ncf_model_train_grad does not cover the model."""
    if kind not in NCF_MODEL_KINDS:
        raise ValueError(f"ncf_model: model kind {kind!r}, covered: {', '.join(map(repr, NCF_MODEL_KINDS))}")
    if factor_num not in NCF_FACTORS:
        raise ValueError(f"ncf_model: factor_num = {factor_num}, covered: {NCF_FACTORS}")
    if not (isinstance(num_layers, (int, np.integer)) and 1 <= num_layers <= NCF_MAX_LAYERS):
        raise ValueError(f"ncf_model: num_layers = {num_layers} outside [1, {NCF_MAX_LAYERS}]")
    if reads_mlp(kind) and factor_num << (num_layers - 1) > NCF_MAX_D:
        raise ValueError(f"ncf_model: d = factor_num * 2^(num_layers - 1) = {factor_num << (num_layers - 1)} above {NCF_MAX_D}")
    eps = float(np.float32(layer_norm_eps))
    if not (np.isfinite(eps) and eps >= 0.0):
        raise ValueError(f"ncf_model: layer_norm_eps = {layer_norm_eps!r} is not finite or negative")


def ncf_model_layout(factor_num: int, num_layers: int, kind: str, use_layer_norm: bool, user_num: int, item_num: int, train_items: bool = True):
    """The flat parameter layout of pmgt_ncf_model_train_grad (include/pmgt_capi.h) -> ({NCF state_dict key: (offset in floats, shape)} in
    buffer order, count), holding only the tensors the kind trains: embed_user_MLP, the two GMF tables, per layer W, b[, gamma, beta],
    predict_layer, and with train_items embed_item_MLP behind them, its offset rounded up to a multiple of 8 floats.  Kind GMF: the two GMF
    tables, then predict_layer.  Every offset but predict_layer.bias's is a multiple of 8 floats."""
    check_ncf_model_covered(factor_num, num_layers, kind)
    if not (isinstance(user_num, (int, np.integer)) and isinstance(item_num, (int, np.integer)) and 1 <= user_num < 2 ** 31 - 1
            and 1 <= item_num < 2 ** 31 - 1):
        raise ValueError(f"ncf_model: user_num = {user_num!r} and item_num = {item_num!r} must be integers in [1, 2^31 - 2]")
    d, user_num, item_num = factor_num << (num_layers - 1), int(user_num), int(item_num)
    mlp, gmf = reads_mlp(kind), reads_gmf(kind)
    shapes = [(USER_MLP, (user_num, d))] if mlp else []
    if gmf:
        shapes += [(USER_GMF, (user_num, factor_num)), (ITEM_GMF, (item_num, factor_num))]
    for i in range(num_layers if mlp else 0):
        out = d >> i
        shapes += list(zip(layer_keys(i, use_layer_norm), [(out, 2 * out), (out,), (out,), (out,)]))
    shapes += [(OUT_W, (1, factor_num * (2 if mlp and gmf else 1))), (OUT_B, (1,))]
    layout, at = {}, 0
    for key, shape in shapes:
        layout[key] = (at, shape)
        at += int(np.prod(shape))
    if mlp and train_items:
        at = (at + 7) // 8 * 8
        layout[ITEM_MLP] = (at, (item_num, d))
        at += item_num * d
    return layout, at


def ncf_model_layout_slots(layout: dict) -> list:
    """The offsets of `layout` in the slot order of pmgt_ncf_model_layout (-1: the kind trains no such tensor).  The Linear of a layer is
    found under either of its two names."""
    out = [layout[k][0] if k in layout else -1 for k in (USER_MLP, USER_GMF, ITEM_GMF)]
    ln = norm_key(0) + ".weight" in layout                   # (MLP_layers.2: layer 0's LayerNorm, or without one its ReLU, which has no tensor)
    for i in range(NCF_MAX_LAYERS):
        out += [layout[k][0] if k in layout else -1 for k in layer_keys(i, ln)] + ([] if ln else [-1, -1])
    out += [layout[k][0] if k in layout else -1 for k in (OUT_W, OUT_B, ITEM_MLP)]
    assert len(out) == NCF_MODEL_TENSORS
    return out


def ncf_model_shape(w: dict, kind: str = None):
    """(factor_num, num_layers, kind, use_layer_norm) of a model given as a state_dict-keyed mapping.  A whole state_dict holds every table
    whatever the kind: `kind` None is then read from predict_layer's width ([1, 2 F]: NeuMF-end) and, for [1, F], from the tables present
    (both families: ambiguous, refused)."""
    factor = int((w[USER_GMF] if USER_GMF in w else w[OUT_W]).shape[-1])
    if kind is None:
        if USER_GMF in w and USER_MLP in w:
            if int(w[OUT_W].shape[-1]) != 2 * factor:
                raise ValueError("ncf_model: the weights hold the GMF and the MLP tables and predict_layer is [1, F]: pass kind= ('MLP' or 'GMF')")
            kind = "NeuMF-end"
        else:
            kind = "GMF" if USER_GMF in w else "MLP"
    if kind not in NCF_MODEL_KINDS:
        raise ValueError(f"ncf_model: model kind {kind!r}, covered: {', '.join(map(repr, NCF_MODEL_KINDS))}")
    if kind == "MLP":
        factor = int(w[OUT_W].shape[-1])
    ln = any(k.startswith("MLP_layers.") and k.endswith(".weight") and np.ndim(v) == 1 for k, v in w.items())
    num_layers = 0
    while linear_key(num_layers, ln) + ".weight" in w:
        num_layers += 1
    if reads_mlp(kind) and num_layers < 1:
        raise ValueError("ncf_model: the weights hold no MLP_layers.0.weight")
    return factor, num_layers, kind, ln


def _mlp_forward(w: dict, users, items, num_layers: int, ln: bool, eps: float, m: dict):
    """The MLP tower: -> (hs = [h_0 .. h_L], per layer (xhat, rstd) with LayerNorm, per layer the pre-ReLU value); m = {site: mask} or {}"""
    x0 = np.concatenate([w[USER_MLP][users], w[ITEM_MLP][items]], axis=1)
    hs, stats, pre = [x0 * m["emb"] if "emb" in m else x0], [], []
    for i in range(num_layers):
        W, b = (w[k] for k in layer_keys(i, ln)[:2])
        a = hs[-1] @ W.T + b
        if f"layer{i}" in m:
            a = a * m[f"layer{i}"]
        if ln:
            a, xhat, rstd = _ln(a, w[norm_key(i) + ".weight"], w[norm_key(i) + ".bias"], eps)
            stats.append((xhat, rstd))
        pre.append(a)
        hs.append(np.maximum(a, 0))
    return hs, stats, pre


def ncf_model_pre_relu(weights: dict, users, items, dtype=np.float64, layer_norm_eps: float = 1e-12, kind: str = None, masks: dict = None) -> list:
    """The pre-ReLU value [n, d >> l] of every layer (kind GMF: []), in eval mode or under `masks`: where the tests look for pairs next to
    the ReLU's kink."""
    w = head_weights(weights, dtype)
    _, num_layers, kind, ln = ncf_model_shape(w, kind)
    if not reads_mlp(kind):
        return []
    return _mlp_forward(w, np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64), num_layers, ln, layer_norm_eps,
                        _masks_as(masks, dtype))[2]


def ncf_model_grad_host(weights: dict, users, items, labels, dtype=np.float64, layer_norm_eps: float = 1e-12, kind: str = None,
                        train_items: bool = True, masks: dict = None):
    """NCF.forward on the pairs (users[p], items[p]), the mean BCE-with-logits loss against `labels` and its gradient, every operation in
    `dtype` -> (loss, logits [n], {state_dict key: gradient}) for every tensor of ncf_model_layout (embed_item_MLP.weight among them when
    train_items).  `weights` is keyed like the NCF class's state_dict (arrays or CPU tensors; tensors the kind never reads may be there and
    are ignored); kind None: ncf_model_shape's reading.  ncf_head._head_grad's rules: the loss is max(z, 0) - z y + log1p(exp(-|z|)),
    dlogit = (sigmoid(z) - y) / n with the sigmoid in its overflow-free form, the ReLU passes where h > 0, and rows of the embedding
    tables hit by several pairs are summed in pair order.
    masks: None, or {site: (bool keep [n, cols], scale)} as ncf_dropout_masks names them ("emb", "gmf", "layer<l>") -- the model in
    TRAINING mode under these masks, and the gradients of that function: dy_l = m_l LNbwd(dh (h > 0)).  A missing site is not dropped."""
    w = head_weights(weights, dtype)
    factor, num_layers, kind, ln = ncf_model_shape(w, kind)
    mlp, gmf = reads_mlp(kind), reads_gmf(kind)
    user_num = len(w[USER_MLP] if mlp else w[USER_GMF])
    item_num = len(w[ITEM_MLP] if mlp else w[ITEM_GMF])
    users, items, y = check_pairs(users, items, labels, user_num, item_num, max_pairs=1 << 40, who="ncf_model")
    y = y.astype(dtype)
    m = _masks_as(masks, dtype)
    n, one = len(users), dtype(1)
    feats = []
    if gmf:
        gu, gi = w[USER_GMF][users], w[ITEM_GMF][items]
        feats.append(gu * gi * m["gmf"] if "gmf" in m else gu * gi)
    if mlp:
        d = w[USER_MLP].shape[1]
        hs, stats, _ = _mlp_forward(w, users, items, num_layers, ln, layer_norm_eps, m)
        feats.append(hs[-1])
    feat = feats[0] if len(feats) == 1 else np.concatenate(feats, axis=1)
    wp = w[OUT_W].reshape(-1)
    z = feat @ wp + w[OUT_B][0]
    e = np.exp(-np.abs(z))
    loss = (np.maximum(z, 0) - z * y + np.log1p(e)).sum(dtype=dtype) / dtype(n)
    dl = (np.where(z >= 0, one / (one + e), e / (one + e)) - y) / dtype(n)
    grads = {OUT_W: (dl @ feat).reshape(1, -1), OUT_B: dl.sum(dtype=dtype).reshape(1)}
    dfeat = dl[:, None] * wp[None, :]
    if gmf:
        dg = dfeat[:, :factor]
        if "gmf" in m:
            dg = dg * m["gmf"]
        grads[USER_GMF], grads[ITEM_GMF] = np.zeros_like(w[USER_GMF]), np.zeros_like(w[ITEM_GMF])
        np.add.at(grads[USER_GMF], users, dg * gi)
        np.add.at(grads[ITEM_GMF], items, dg * gu)
    if mlp:
        dh = dfeat[:, factor:] if gmf else dfeat
        for i in reversed(range(num_layers)):
            keys = layer_keys(i, ln)
            dz = dh * (hs[i + 1] > 0)
            if ln:
                xhat, rstd = stats[i]
                grads[keys[2]] = (dz * xhat).sum(axis=0, dtype=dtype)
                grads[keys[3]] = dz.sum(axis=0, dtype=dtype)
                dz = _ln_bwd(dz, w[keys[2]], xhat, rstd)
            if f"layer{i}" in m:
                dz = dz * m[f"layer{i}"]
            grads[keys[0]] = dz.T @ hs[i]
            grads[keys[1]] = dz.sum(axis=0, dtype=dtype)
            dh = dz @ w[keys[0]]
        if "emb" in m:
            dh = dh * m["emb"]
        grads[USER_MLP] = np.zeros_like(w[USER_MLP])
        np.add.at(grads[USER_MLP], users, dh[:, :d])
        if train_items:
            grads[ITEM_MLP] = np.zeros_like(w[ITEM_MLP])
            np.add.at(grads[ITEM_MLP], items, dh[:, d:])
    assert all(g.dtype == dtype for g in grads.values()) and z.dtype == dtype
    return dtype(loss), z, grads


def ncf_model_scores_host(weights: dict, users, table=None, dtype=np.float64, layer_norm_eps: float = 1e-12, kind: str = None) -> np.ndarray:
    """NCF.head in eval mode for every user of `users` against the whole catalogue -> logits [len(users), I] with (users[r], item j) at
    [r, j], every operation in `dtype`, layer 0 on the UNSPLIT concatenation: the yardstick of pmgt_ncf_model_score.  The pair rows are those
    of ncf_model_grad_host on users = repeat(users, I), items = tile(arange(I), n), so the logits are that function's, bit for bit.
    `weights` is keyed like the NCF class's state_dict; `table` [I, d] stands in for embed_item_MLP.weight (None: that tensor).  Kind GMF
    reads no MLP tensor and refuses a `table`; NeuMF-pre is scored as NeuMF-end."""
    w = head_weights(weights, dtype)
    _, num_layers, kind, ln = ncf_model_shape(w, kind)
    mlp, gmf = reads_mlp(kind), reads_gmf(kind)
    if mlp and table is not None:
        w[ITEM_MLP] = np.asarray(table.detach().cpu().numpy() if hasattr(table, "detach") else table).astype(dtype)
    elif table is not None:
        raise ValueError("ncf_model: kind 'GMF' reads no item table")
    n_items = len(w[ITEM_MLP] if mlp else w[ITEM_GMF])
    if gmf and len(w[ITEM_GMF]) < n_items:
        raise ValueError("ncf_model: embed_item_GMF.weight has fewer rows than the item table")
    users = np.asarray(users, dtype=np.int64)
    if users.ndim != 1 or (len(users) and not (0 <= users.min() and users.max() < len(w[USER_MLP] if mlp else w[USER_GMF]))):
        raise ValueError("ncf_model: users must be one-dimensional ids inside the user tables")
    n = len(users)
    pu, pi = np.repeat(users, n_items), np.tile(np.arange(n_items, dtype=np.int64), n)
    feats = []
    if gmf:
        feats.append(w[USER_GMF][pu] * w[ITEM_GMF][pi])
    if mlp:
        feats.append(_mlp_forward(w, pu, pi, num_layers, ln, layer_norm_eps, {})[0][-1])
    feat = feats[0] if len(feats) == 1 else np.concatenate(feats, axis=1)
    z = feat @ w[OUT_W].reshape(-1) + w[OUT_B][0]
    assert z.dtype == dtype
    return z.reshape(n, n_items)
