"""What the reference's Deep & Cross Network is (pmgt/dcn/models.py), stated once for the model class (dcn.py), the training and the
evaluation (dcn_train.py): which shapes the kernels cover, the flat parameter layout of pmgt_dcn_train_grad, the refusals, and the two
numpy references every DCN kernel is judged against (dcn_head_host: logits; dcn_head_grad_host: loss, logits and every gradient).
With E = F 2^L the embedding width and D = 2 E:
  x0 = [user_embeddings[u] ; item_embeddings[i]]
  cross   x^(0) = x0,  s_c = x^(c) . w_c,  x^(c+1) = LN_c(x0 s_c + x0)            (the layer adds x0, NOT x^(c); its `bias` is never read)
  deep    h_0 = x0,  h_(l+1) = relu(LN_l(W_l h_l + b_l)),  W_l [D >> (l + 1)][D >> l]
  z = output_layer.weight . [x^(C) ; h_L] + output_layer.bias,   loss = mean BCE-with-logits
LN is torch.nn.LayerNorm (biased variance, (x - mean) / sqrt(var + eps) gamma + beta), absent without use_layer_norm.
IN TRAINING MODE (pmgt_dcn_train_grad_dropout; masks m = 0 or 1 / (1 - p) per element, dcn_dropout_masks):
  x0 = m_e [user ; item],   x^(c+1) = LN_c(m_c (x0 s_c) + x0),   h_(l+1) = relu(LN_l(m_l (W_l h_l + b_l)))
the added x0 is the dropped x0, not masked again, and the deep dropout sits BEFORE the LayerNorm (dropped zeros enter its statistics).
What the DCN shares with the other pair head, the NCF head -- the id and pair checks, head_weights, the dropout RNG -- lives in pair_train.py.

SCORED AGAINST THE WHOLE CATALOGUE (dcn_scores_host: the yardstick, by the formulae above on pair rows; pmgt_dcn_score: the kernel, by the
form below).  The deep net is the NCF tower with layer 0 split into a per-user and a per-item product.  The cross net COLLAPSES, because the
layer adds x0: every cross state is a scalar multiple of x0 (no LayerNorm) or an affine image of the centred x0 (LayerNorm), so every s_c
and the output dot split into one scalar per user row plus one per item row.  With wo = output_layer.weight, w_C := wo[:D], the "half" of a
D-vector [0, E) for a user row and [E, D) for an item row, and for a table row v of a half
    d_c(v) = sum_j v_j g_c[j],   g_0 = w_0[half],   g_c = w_c[half] (no LayerNorm)  or  gamma_(c-1)[half] * w_c[half] (LayerNorm),  c = 1 .. C:
  without LayerNorm   a = 1;   for c = 0 .. C-1:  a = a (d_c(u) + d_c(i)) + 1;   z_cross = a (d_C(u) + d_C(i))
  with LayerNorm      mu(v) the row mean, q(v) = sum_j (v_j - mu(v))^2,
                      m0 = (mu(u) + mu(i)) / 2,   v0 = (q(u) + q(i) + E ((mu(u) - m0)^2 + (mu(i) - m0)^2)) / D      (pooled; no E[x^2] - m^2)
                      s = d_0(u) + d_0(i);   for c = 0 .. C-1:  k = s + 1,  t = k / sqrt(k^2 v0 + eps),
                                                                s = t (d_(c+1)(u) + d_(c+1)(i) - m0 K_c) + B_c;      z_cross = s
                      K_c = sum_D gamma_c w_(c+1),  B_c = sum_D beta_c w_(c+1):  2 C constants of the model
  z = (z_cross + wo[D:] . h_L) + output_layer.bias
About 6 C flops a pair instead of 6 C D, and nothing D-wide is formed per pair outside the deep tower.  dcn_score_constants and
dcn_row_scalars_host state K_c, B_c, g_c and the row scalars in numpy (the yardstick of pmgt_dcn_score_rows).
Pure numpy and the bindings module: importing this loads no GPU library."""
import numpy as np

from ._lib import (DCN_FACTORS, DCN_MAX_CROSS, DCN_MAX_DEEP, DCN_MAX_E, DCN_MAX_PAIRS, DCN_SITE_CROSS, DCN_SITE_DEEP, DCN_SITE_EMB,
                   DCN_TENSORS)
from .pair_train import check_dropout_p, check_ids, check_pairs, dropout_keep, dropout_scale, head_weights, per_layer

ncf_dropout_keep, ncf_dropout_scale = dropout_keep, dropout_scale      # (the names they were imported under before pair_train.py)

USER_KEY, ITEM_KEY = "user_embeddings.weight", "item_embeddings.weight"
OUT_W, OUT_B = "output_layer.weight", "output_layer.bias"


def deep_keys(l: int, use_layer_norm: bool) -> list:
    p = f"deep_net.layers.{l}."
    return [p + "linear.weight", p + "linear.bias"] + ([p + "layer_norm.weight", p + "layer_norm.bias"] if use_layer_norm else [])


def cross_keys(c: int, use_layer_norm: bool) -> list:
    """The TRAINED tensors of cross layer c: `cross_net.layers.c.bias` is a parameter the forward never reads, so it is not among them."""
    p = f"cross_net.layers.{c}."
    return [p + "weight"] + ([p + "layer_norm.weight", p + "layer_norm.bias"] if use_layer_norm else [])


def check_dcn_covered(factor_num: int, deep_layers: int, cross_layers: int) -> None:
    """ValueError naming the limit when the kernels (pmgt_dcn_forward, pmgt_dcn_train_grad) do not cover the shape."""
    if factor_num not in DCN_FACTORS:
        raise ValueError(f"dcn: factor_num = {factor_num}, covered: {DCN_FACTORS}")
    if not (isinstance(deep_layers, (int, np.integer)) and 1 <= deep_layers <= DCN_MAX_DEEP):
        raise ValueError(f"dcn: deep_net_num_layers = {deep_layers} outside [1, {DCN_MAX_DEEP}]")
    if factor_num << deep_layers > DCN_MAX_E:
        raise ValueError(f"dcn: embedding width factor_num * 2^deep_net_num_layers = {factor_num << deep_layers} above {DCN_MAX_E}")
    if not (isinstance(cross_layers, (int, np.integer)) and 1 <= cross_layers <= DCN_MAX_CROSS):
        raise ValueError(f"dcn: cross_net_num_layers = {cross_layers} outside [1, {DCN_MAX_CROSS}]")


def check_dcn_dropout(emb_dropout: float, dropout: float) -> None:
    if emb_dropout != 0 or dropout != 0:
        raise ValueError(f"dcn: dropout is not covered (emb_dropout = {emb_dropout}, dropout = {dropout}): the trainer, the fit and the "
                         "evaluation are eval-mode arithmetic; set both to 0")


def check_dcn_p(p, what: str) -> float:
    """check_dropout_p in the DCN's name."""
    return check_dropout_p(p, what, "dcn")


def dcn_per_layer(p_deep, p_cross, deep: int, cross: int):
    """(one p per deep layer, one per cross layer) of settings that are one p or a sequence each; the refusal of a sequence of another
    length names both counts."""
    n_deep, n_cross = (count if np.isscalar(p) else len(p) for p, count in ((p_deep, deep), (p_cross, cross)))
    what = f"{n_deep} deep and {n_cross} cross dropouts for {deep} deep and {cross} cross layers"
    return per_layer(p_deep, deep, what, "dcn"), per_layer(p_cross, cross, what, "dcn")


def dcn_dropout_masks(seed: int, step: int, n: int, factor: int, deep: int, cross: int, p_emb: float, p_deep, p_cross) -> dict:
    """The masks pmgt_dcn_train_grad_dropout draws for a call on `n` pairs -> {site name: (bool keep [n, cols], fp32 scale)}: "emb" [n, D]
    (the user half first), "deep<l>" [n, D >> (l + 1)] and "cross<c>" [n, D], by the hash pair_train.dropout_keep restates (one RNG for
    every kernel of the project) at the sites DCN_SITE_EMB, DCN_SITE_DEEP + l, DCN_SITE_CROSS + c; row = the pair's index within the call.
    p_deep / p_cross: one p for every layer or a sequence of one per layer.  What dcn_head_grad_host(masks=...) applies."""
    check_dcn_covered(factor, deep, cross)
    p_deep, p_cross = dcn_per_layer(p_deep, p_cross, deep, cross)
    for what, p in [("emb_dropout", p_emb)] + [(f"the dropout of deep layer {l}", p) for l, p in enumerate(p_deep)] + \
            [(f"the dropout of cross layer {c}", p) for c, p in enumerate(p_cross)]:
        check_dcn_p(p, what)
    D = 2 * (factor << deep)
    masks = {"emb": (dropout_keep(seed, step, DCN_SITE_EMB, n, D, p_emb), dropout_scale(p_emb))}
    for l in range(deep):
        masks[f"deep{l}"] = (dropout_keep(seed, step, DCN_SITE_DEEP + l, n, D >> (l + 1), p_deep[l]), dropout_scale(p_deep[l]))
    for c in range(cross):
        masks[f"cross{c}"] = (dropout_keep(seed, step, DCN_SITE_CROSS + c, n, D, p_cross[c]), dropout_scale(p_cross[c]))
    return masks


def _mask(masks, site: str, dtype):
    """keep * scale of `site` in `dtype`, or None: no mask (masks None, or the site missing)"""
    if masks is None or site not in masks:
        return None
    keep, scale = masks[site]
    return np.asarray(keep).astype(dtype) * dtype(scale)


def dcn_shape(weights: dict):
    """(factor_num, deep_layers, cross_layers, use_layer_norm) of a DCN given as a state_dict-keyed mapping."""
    L = C = 0
    while f"deep_net.layers.{L}.linear.weight" in weights:
        L += 1
    while f"cross_net.layers.{C}.weight" in weights:
        C += 1
    if L < 1 or C < 1:
        raise ValueError("dcn: the weights hold no deep_net.layers.0.linear.weight or no cross_net.layers.0.weight")
    E = int(weights[USER_KEY].shape[1])
    return E >> L, L, C, "deep_net.layers.0.layer_norm.weight" in weights


def dcn_layout(factor_num: int, deep_layers: int, cross_layers: int, use_layer_norm: bool, user_num: int, item_num: int):
    """The flat parameter layout of pmgt_dcn_train_grad (include/pmgt_capi.h) -> ({state_dict key: (offset in floats, shape)} in buffer
    order, parameter count): the user table, the item table, per deep layer W, b[, gamma, beta], per cross layer w[, gamma, beta], then
    output_layer.weight and .bias.  Every tensor but the last (one float) has a multiple of 8 floats, so every offset is 32-byte aligned.
    cross_net.layers.c.bias is not in it: it is never read, gets no gradient and is never stepped."""
    check_dcn_covered(factor_num, deep_layers, cross_layers)
    if not (isinstance(user_num, (int, np.integer)) and isinstance(item_num, (int, np.integer)) and 1 <= user_num < 2 ** 31 - 1
            and 1 <= item_num < 2 ** 31 - 1):
        raise ValueError(f"dcn: user_num = {user_num!r} and item_num = {item_num!r} must be integers in [1, 2^31 - 2]")
    E = factor_num << deep_layers
    D = 2 * E
    shapes = [(USER_KEY, (int(user_num), E)), (ITEM_KEY, (int(item_num), E))]
    for l in range(deep_layers):
        out, inn = D >> (l + 1), D >> l
        shapes += list(zip(deep_keys(l, use_layer_norm), [(out, inn), (out,), (out,), (out,)]))
    for c in range(cross_layers):
        shapes += list(zip(cross_keys(c, use_layer_norm), [(D, 1), (D,), (D,)]))
    shapes += [(OUT_W, (1, D + 2 * factor_num)), (OUT_B, (1,))]
    layout, at = {}, 0
    for key, shape in shapes:
        layout[key] = (at, shape)
        at += int(np.prod(shape))
    return layout, at


def dcn_layout_slots(layout: dict) -> list:
    """The offsets of `layout` in the slot order of pmgt_dcn_layout: DCN_TENSORS = 38 slots, -1 for a tensor the model does not have."""
    slots = [USER_KEY, ITEM_KEY]
    for l in range(DCN_MAX_DEEP):
        slots += deep_keys(l, True)
    for c in range(DCN_MAX_CROSS):
        slots += cross_keys(c, True)
    slots += [OUT_W, OUT_B]
    assert len(slots) == DCN_TENSORS
    return [layout[k][0] if k in layout else -1 for k in slots]


def decays(key: str) -> bool:
    """get_optimizer's rule (pmgt/base_trainer.py:35-58, no_decay = ["bias", "LayerNorm.weight"]) on the DCN's names: its LayerNorms are
    called `layer_norm`, so their weights DO decay; a tensor decays unless its name contains "bias"."""
    return "bias" not in key


def check_dcn_pairs(users, items, labels, user_num: int, item_num: int):
    """check_pairs with the DCN entries' limit of pairs a call."""
    return check_pairs(users, items, labels, user_num, item_num, max_pairs=DCN_MAX_PAIRS, who="dcn")


def _ln(u, gamma, beta, eps):
    mean = u.mean(axis=1, keepdims=True)
    cen = u - mean
    rstd = u.dtype.type(1) / np.sqrt((cen * cen).mean(axis=1, keepdims=True) + u.dtype.type(eps))
    xhat = cen * rstd
    return xhat * gamma + beta, xhat, rstd


def _ln_bwd(gy, gamma, xhat, rstd):
    gp = gy * gamma
    return rstd * (gp - gp.mean(axis=1, keepdims=True) - xhat * (gp * xhat).mean(axis=1, keepdims=True))


def _forward(w: dict, users, items, eps: float, masks: dict = None):
    """Everything the backward needs: x0, the cross states xs [x^(0) .. x^(C)] with (xhat, rstd) per layer, the deep states.
    masks: None (eval mode, today's bits) or dcn_dropout_masks' dict: x0 is then the DROPPED x0 and deep[l][0] the LayerNorm's output
    over the dropped Linear output."""
    _, L, C, ln = dcn_shape(w)
    x0 = np.concatenate([w[USER_KEY][users], w[ITEM_KEY][items]], axis=1)
    dtype = x0.dtype.type
    m = _mask(masks, "emb", dtype)
    if m is not None:
        x0 = x0 * m
    xs, cross = [x0], []
    for c in range(C):
        s = xs[-1] @ w[f"cross_net.layers.{c}.weight"].reshape(-1)
        m = _mask(masks, f"cross{c}", dtype)
        u = x0 * s[:, None] + x0 if m is None else (x0 * s[:, None]) * m + x0
        if ln:
            p = f"cross_net.layers.{c}.layer_norm."
            y, xhat, rstd = _ln(u, w[p + "weight"], w[p + "bias"], eps)
        else:
            y, xhat, rstd = u, None, None
        xs.append(y)
        cross.append((s, xhat, rstd))
    hs, deep = [x0], []
    for l in range(L):
        p = f"deep_net.layers.{l}."
        a = hs[-1] @ w[p + "linear.weight"].T + w[p + "linear.bias"]
        m = _mask(masks, f"deep{l}", dtype)
        if m is not None:
            a = a * m
        if ln:
            a, xhat, rstd = _ln(a, w[p + "layer_norm.weight"], w[p + "layer_norm.bias"], eps)
        else:
            xhat = rstd = None
        hs.append(np.maximum(a, 0))
        deep.append((a, xhat, rstd))
    feat = np.concatenate([xs[-1], hs[-1]], axis=1)
    z = feat @ w[OUT_W].reshape(-1) + w[OUT_B][0]
    return x0, xs, cross, hs, deep, feat, z


def dcn_head_host(weights: dict, users, items, dtype=np.float64, layer_norm_eps: float = 1e-12) -> np.ndarray:
    """DCN.forward in eval mode on plain arrays -> logits [n] in `dtype`.  `weights` is keyed like the model's state_dict (arrays or CPU
    tensors); the LayerNorm is on when its keys are there."""
    w = head_weights(weights, dtype)
    users, items = np.asarray(users, dtype=np.int64), np.asarray(items, dtype=np.int64)
    check_ids("users", users, len(w[USER_KEY]), "dcn")
    check_ids("items", items, len(w[ITEM_KEY]), "dcn")
    return _forward(w, users, items, layer_norm_eps)[-1]


def dcn_head_grad_host(weights: dict, users, items, labels, dtype=np.float64, layer_norm_eps: float = 1e-12, masks: dict = None):
    """DCN.forward with dropout 0 on the pairs (users[p], items[p]), the mean BCE-with-logits loss against `labels` and its gradient, every
    operation in `dtype` -> (loss, logits [n], {state_dict key: gradient}) for every tensor of dcn_layout (the cross layers' unused `bias`
    has no gradient).  The loss is max(z, 0) - z y + log1p(exp(-|z|)), dz = (sigmoid(z) - y) / n with the sigmoid in its overflow-free
    form, the ReLU passes where h > 0, and embedding rows hit by several pairs are summed in pair order (np.add.at).
    masks: None, or {site: (bool keep [n, cols], scale)} as dcn_dropout_masks names them -- the model in TRAINING mode under these masks,
    m = keep * scale in `dtype` (the module's header), and the gradients of that function: dy_l = m_l LNbwd(..), ds_c = sum_j g_j m_cj x0_j,
    d x0 += g (m_c s_c) + g, and d x0 carries m_e to the embedding rows.  A site that is missing is not dropped; None keeps today's bits."""
    w = head_weights(weights, dtype)
    F, L, C, ln = dcn_shape(w)
    users, items, y = check_pairs(users, items, labels, len(w[USER_KEY]), len(w[ITEM_KEY]), max_pairs=1 << 40)
    y = y.astype(dtype)
    n, one = len(users), dtype(1)
    x0, xs, cross, hs, deep, feat, z = _forward(w, users, items, layer_norm_eps, masks)
    D = x0.shape[1]
    e = np.exp(-np.abs(z))
    loss = (np.maximum(z, 0) - z * y + np.log1p(e)).sum(dtype=dtype) / dtype(n)
    dl = (np.where(z >= 0, one / (one + e), e / (one + e)) - y) / dtype(n)
    wo = w[OUT_W].reshape(-1)
    grads = {OUT_W: (dl @ feat).reshape(1, -1), OUT_B: dl.sum(dtype=dtype).reshape(1)}
    dfeat = dl[:, None] * wo[None, :]
    g, dx0 = dfeat[:, :D], np.zeros_like(x0)
    for c in reversed(range(C)):
        s, xhat, rstd = cross[c]
        p = f"cross_net.layers.{c}."
        if ln:
            grads[p + "layer_norm.weight"] = (g * xhat).sum(axis=0, dtype=dtype)
            grads[p + "layer_norm.bias"] = g.sum(axis=0, dtype=dtype)
            g = _ln_bwd(g, w[p + "layer_norm.weight"], xhat, rstd)
        m = _mask(masks, f"cross{c}", dtype)
        gm = g if m is None else g * m                       # d loss / d (x0 s_c)
        ds = (gm * x0).sum(axis=1, dtype=dtype)
        dx0 = dx0 + (gm * s[:, None] + g)
        grads[p + "weight"] = (ds @ xs[c]).reshape(-1, 1)
        g = ds[:, None] * w[p + "weight"].reshape(-1)[None, :]
    dx0 = dx0 + g                                            # x^(0) is x0
    dh = dfeat[:, D:]
    for l in reversed(range(L)):
        a, xhat, rstd = deep[l]
        p = f"deep_net.layers.{l}."
        da = dh * (hs[l + 1] > 0)
        if ln:
            grads[p + "layer_norm.weight"] = (da * xhat).sum(axis=0, dtype=dtype)
            grads[p + "layer_norm.bias"] = da.sum(axis=0, dtype=dtype)
            da = _ln_bwd(da, w[p + "layer_norm.weight"], xhat, rstd)
        m = _mask(masks, f"deep{l}", dtype)
        if m is not None:
            da = da * m
        grads[p + "linear.weight"] = da.T @ hs[l]
        grads[p + "linear.bias"] = da.sum(axis=0, dtype=dtype)
        dh = da @ w[p + "linear.weight"]
    dx0 = dx0 + dh
    m = _mask(masks, "emb", dtype)
    if m is not None:
        dx0 = dx0 * m
    E = D // 2
    grads[USER_KEY], grads[ITEM_KEY] = np.zeros_like(w[USER_KEY]), np.zeros_like(w[ITEM_KEY])
    np.add.at(grads[USER_KEY], users, dx0[:, :E])
    np.add.at(grads[ITEM_KEY], items, dx0[:, E:])
    assert all(v.dtype == dtype for v in grads.values()) and z.dtype == dtype
    return dtype(loss), z, grads


def dcn_scores_host(weights: dict, users, table=None, dtype=np.float64, layer_norm_eps: float = 1e-12, pair_chunk: int = 1 << 16) -> np.ndarray:
    """DCN.forward in eval mode for every user of `users` against the whole catalogue -> logits [len(users), I] in `dtype` with (users[r],
    item j) at [r, j]: the yardstick of pmgt_dcn_score.  _forward on the pair rows users = repeat(u, I), items = tile(arange(I), len(u)) of
    chunks u of whole users (about pair_chunk pairs each), so a block is dcn_head_host's logits of those pair rows, bit for bit.
    `table` [I, E] stands in for item_embeddings.weight (None: that tensor)."""
    w = head_weights(weights, dtype)
    if table is not None:
        table = np.asarray(table.detach().cpu().numpy() if hasattr(table, "detach") else table).astype(dtype)
        if table.ndim != 2 or table.shape[1] != w[USER_KEY].shape[1] or len(table) < 1:
            raise ValueError(f"dcn: the item table {table.shape} must be [I >= 1, E = {w[USER_KEY].shape[1]}]")
        w[ITEM_KEY] = table
    users = np.asarray(users, dtype=np.int64)
    if users.ndim != 1:
        raise ValueError(f"dcn: users {users.shape} must be one-dimensional")
    check_ids("users", users, len(w[USER_KEY]), "dcn")
    n, n_items = len(users), len(w[ITEM_KEY])
    out = np.empty((n, n_items), dtype=dtype)
    per = max(1, int(pair_chunk) // n_items)
    item_ids = np.arange(n_items, dtype=np.int64)
    for lo in range(0, n, per):
        u = users[lo: lo + per]
        out[lo: lo + len(u)] = _forward(w, np.repeat(u, n_items), np.tile(item_ids, len(u)), layer_norm_eps)[-1].reshape(len(u), n_items)
    return out


def dcn_score_constants(weights: dict, dtype=np.float64):
    """The model constants of the collapsed cross net (the module's header) -> (g [2][C + 1][E]: g_c of the user half and of the item half,
    K [C], B [C]); K and B are zeros without LayerNorm."""
    w = head_weights(weights, dtype)
    _, _, C, ln = dcn_shape(w)
    E = w[USER_KEY].shape[1]
    D = 2 * E
    ws = [w[f"cross_net.layers.{c}.weight"].reshape(-1) for c in range(C)] + [w[OUT_W].reshape(-1)[:D]]
    g, K, B = np.empty((2, C + 1, E), dtype=dtype), np.zeros(C, dtype=dtype), np.zeros(C, dtype=dtype)
    for c in range(C + 1):
        full = ws[c]
        if ln and c:
            p = f"cross_net.layers.{c - 1}.layer_norm."
            full = w[p + "weight"] * ws[c]
            K[c - 1], B[c - 1] = full.sum(dtype=dtype), (w[p + "bias"] * ws[c]).sum(dtype=dtype)
        g[0, c], g[1, c] = full[:E], full[E:]
    return g, K, B


def dcn_row_scalars_host(weights: dict, rows, half: int, dtype=np.float64) -> np.ndarray:
    """What pmgt_dcn_score_rows writes for the table rows `rows` [m, E] of `half` (0: users, 1: items) -> [m, C + 3] = mu, q, d_0 .. d_C;
    mu and q are 0 without LayerNorm."""
    _, _, C, ln = dcn_shape(weights)
    g = dcn_score_constants(weights, dtype)[0][half]
    v = np.asarray(rows, dtype=dtype)
    out = np.zeros((len(v), C + 3), dtype=dtype)
    if ln:
        mu = v.mean(axis=1)
        out[:, 0], out[:, 1] = mu, ((v - mu[:, None]) ** 2).sum(axis=1)
    out[:, 2:] = v @ g.T
    return out
