"""Shared by the tests of the stand-alone NCF model: the fixture, seeded models, the numpy yardstick in both precisions, and the choice of
well-conditioned pairs.

THE MEASURE is tests/dcn_util.py's (ratios, C_BOUND), per quantity (loss, logits, each gradient tensor), o64 / r32 = ncf_model_grad_host in
fp64 / fp32:   max|x - o64| <= C max(max|r32 - o64|, 2^-22 max|o64|),   C = 4.  This model has no degenerate tensor.

WELL-CONDITIONED PAIRS, chosen on the host before the device computes anything: a pair is drawn again when a LayerNorm output (the pre-ReLU
value) of its row lies within 8 x the fp32-numpy error of its layer from 0 (the ReLU is discontinuous there); at most 1 pair in 8 of a case
may be drawn again (world() asserts it for every n of NS).

THE ONE LOGIT OF n = 1.  A case of one pair has one logit, z = sum_f wp_f feat_f + b, and its floor is 2^-22 |z|.  Where that sum cancels,
the floor falls below 2^-24 sum_f |wp_f feat_f|, one rounding unit of the terms: no fp32 sum in another order than numpy's can be expected
to meet it, so such a list judges the order of a sum and not its correctness (tests/dcn_dropout_util.py notes the same of the DCN's lists).
PAIR_SEEDS / DROP_PAIR_SEEDS: per model the first seed from 29 on at which the cap holds for every n of NS and the first pair's logit keeps
|z| >= 2^-3 (sum_f |wp_f feat_f| + |b|) -- in eval mode and, for the dropout lists, under every mask set --, so that the bound of the
n = 1 case, 4 x its floor, is at least two rounding units of its terms (at 2^-2 the four-layer model, whose 24 distinct pairs all cancel
under one mask set or another, has no list).

THE SUM OF THE dlogits.  d loss / d predict_layer.bias = sum_p dlogit_p is one number too, and with mixed labels its terms have both
signs: the same argument and the same threshold, |sum_p dlogit_p| >= 2^-3 sum_p |dlogit_p| for every n of NS (all 0 / all 1 labels have one
sign and cannot cancel).  Every other quantity is a tensor judged by its largest element, or a sum of non-negative terms (the loss).
A SECOND AND A THIRD REALISATION.  A list on which a right fp32 realisation misses the bound cannot judge a kernel (a pre-LayerNorm row of
small variance, a sum that cancels: tests/dcn_dropout_util.py says the same of the DCN's lists).  HEADS and DROP_HEADS therefore take the
first seed at which, besides the above, two more fp32 realisations keep within C on every case of the GPU test: torch autograd through
pmgt_amd.ncf.NCF (torch_grad, torch_grad_masked) and the numpy yardstick IN ANOTHER ORDER OF SUMS (permuted_host: the columns of every
table and the units of every layer permuted, three permutations).  (The dropout list of (8, 2, NeuMF-end) at seed 33 passes everything
else, and the permuted yardstick misses the bound on d embed_user_MLP by 10.9 x at n = 130: that list judges nothing.)
All of it is decided on the CPU by the yardstick's realisations alone (python -m tests.ncf_model_util prints the search); world() asserts
the cap and the two conditions before the device computes anything, tests/test_ncf_model_measure_cpu.py the realisations."""
import functools
import os

import numpy as np
import torch

from pmgt_amd.ncf_head import ncf_dropout_masks
from pmgt_amd.ncf_model import ncf_model_grad_host, ncf_model_layout, ncf_model_pre_relu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, "tests", "golden", "ncf_model.npz"))
TAGS = ("mlp_ln", "neumf_ln", "gmf", "neumf_noln", "pre")

# (factor_num, num_layers, kind, LayerNorm): d = 8, below the 32-wide block; NeuMF; widths 64 / 32 / 16; d = 256, the widest; four layers; GMF
HEADS = [(8, 1, "MLP", True), (8, 2, "NeuMF-end", True), (16, 3, "MLP", True), (64, 3, "NeuMF-end", True), (32, 4, "MLP", True),
         (8, 2, "GMF", False), (64, 1, "GMF", False)]
# further models of the tests: without LayerNorm (the bits of the PMGT_NCF head's kernels), and what the trainer tests build
OTHER_HEADS = [(16, 3, "NeuMF-end", False), (8, 2, "MLP", False), (8, 2, "NeuMF-pre", False), (16, 3, "MLP", False), (8, 2, "MLP", True),
               (8, 2, "GMF", True)]
NS = (1, 31, 33, 130)
USER_NUM, ITEM_NUM = 5, 7
EPS = 1e-12
# the pair lists (chosen on the CPU: python -m tests.ncf_model_util)
PAIR_SEEDS = {(8, 1, "MLP", True): 29, (8, 2, "NeuMF-end", True): 30, (16, 3, "MLP", True): 29, (64, 3, "NeuMF-end", True): 31,
              (32, 4, "MLP", True): 31, (8, 2, "GMF", False): 29, (64, 1, "GMF", False): 30, (16, 3, "NeuMF-end", False): 31,
              (8, 2, "MLP", False): 29, (8, 2, "NeuMF-pre", False): 29, (16, 3, "MLP", False): 29, (8, 2, "MLP", True): 29, (8, 2, "GMF", True): 29}
DROP_PAIR_SEEDS = {(8, 2, "NeuMF-end", True): 44, (16, 3, "MLP", True): 29, (32, 4, "MLP", True): 105, (8, 2, "GMF", False): 29}
FIRST_LOGIT = 0.125                                         # the least |z| / (sum |terms| + |b|) of the first pair: see the header


def head_id(h):
    return f"f{h[0]}-L{h[1]}-{h[2]}-{'ln' if h[3] else 'noln'}"


def fixture(tag):
    """(weights, gradients, users, items, labels, (factor, layers, kind, ln)) of a tag of tests/golden/ncf_model.npz"""
    w = {str(k): GOLD[f"{tag}/w/{k}"] for k in GOLD[tag + "/keys"]}
    g = {k[len(tag) + 3:]: GOLD[k] for k in GOLD.files if k.startswith(tag + "/g/")}
    factor, layers, ln = (int(v) for v in GOLD[tag + "/shape"])
    return w, g, GOLD[tag + "/users"], GOLD[tag + "/items"], GOLD[tag + "/labels"], (factor, layers, str(GOLD[tag + "/kind"]), bool(ln))


def random_model(factor, layers, kind, ln, user_num, item_num, seed):
    """The trained tensors of an NCF as fp32 numpy arrays keyed like the state_dict, every one away from its init's special values
    (gamma != 1, beta != 0, biases != 0), scaled so that the logits stay O(1)."""
    rng = np.random.default_rng(seed)
    layout, _ = ncf_model_layout(factor, layers, kind, ln, user_num, item_num, True)
    w = {}
    for key, (_, shape) in layout.items():
        v = rng.standard_normal(shape)
        if key.startswith("embed_"):
            v *= 1.0 if ln or kind == "GMF" else 0.5
        elif len(shape) == 2:                                # a Linear's weight
            v *= 1.0 / np.sqrt(shape[1])
        elif key.endswith(".weight"):                        # a LayerNorm's gamma
            v = 1.0 + 0.3 * v
        else:
            v *= 0.3
        w[key] = v.astype(np.float32)
    return w


def flatten(w, layout, count):
    flat = np.zeros(count, dtype=np.float32)
    for key, (off, shape) in layout.items():
        flat[off: off + w[key].size] = w[key].reshape(-1)
    return flat


def split(loss, logits, grads, layout):
    g = grads.cpu().numpy()
    out = {"loss": loss.cpu().numpy(), "logits": logits.cpu().numpy()}
    out.update({k: g[off: off + int(np.prod(shape))].reshape(shape) for k, (off, shape) in layout.items()})
    return out


def host(w, kind, users, items, labels, dtype, train_items=True, masks=None):
    loss, logits, grads = ncf_model_grad_host(w, users, items, labels, dtype, layer_norm_eps=EPS, kind=kind, train_items=train_items, masks=masks)
    return dict(grads, loss=np.asarray([loss]), logits=logits)


def torch_model(w, shape, dtype=torch.float32, device="cpu", user_num=None, item_num=None, **kwargs):
    """A pmgt_amd.ncf.NCF holding `w` (tensors the kind never reads keep their init)."""
    from pmgt_amd.ncf import NCF
    factor, layers, kind, ln = shape
    user_num = user_num or len(w["embed_user_MLP.weight"] if "embed_user_MLP.weight" in w else w["embed_user_GMF.weight"])
    item_num = item_num or len(w["embed_item_MLP.weight"] if "embed_item_MLP.weight" in w else w["embed_item_GMF.weight"])
    model = NCF(user_num, item_num, factor, layers, use_layer_norm=ln, layer_norm_eps=EPS, model=kind, **kwargs).to(dtype)
    missing = model.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in w.items()}, strict=False)
    assert not missing.unexpected_keys
    return model.to(device)


SEED = 0x1234_5678_9ABC                                      # of the dropout tests (above 2^32: both halves of the seed take part)


def masks_of(shape, n, p_emb, p_layer, step, seed=SEED):
    """ncf_dropout_masks for a model of `shape`; kind GMF draws the gmf site alone"""
    factor, layers, kind, _ = shape
    masks = ncf_dropout_masks(seed, step, n, factor, layers, "MLP" if kind == "MLP" else "NeuMF-end", p_emb, p_layer)
    return {"gmf": masks["gmf"]} if kind == "GMF" else masks


def cut(masks, n):
    """the first n rows of every site (a site's row is the pair's index)"""
    return {k: (keep[:n], scale) for k, (keep, scale) in masks.items()}


def ill_conditioned(w, kind, users, items, masks=None):
    """bool [n]: the pairs the header's rule draws again (under `masks`: the rule on the training-mode forward)"""
    bad = np.zeros(len(users), dtype=bool)
    for a64, a32 in zip(ncf_model_pre_relu(w, users, items, np.float64, EPS, kind, masks), ncf_model_pre_relu(w, users, items, np.float32, EPS, kind, masks)):
        bad |= ~(np.abs(a64).min(axis=1) > 8 * np.abs(a32 - a64).max())
    return bad


def first_logit_condition(w, kind, users, items, masks=None) -> float:
    """|z| / (sum_f |wp_f feat_f| + |b|) of the first pair in fp64: how far its logit is from cancelling"""
    from pmgt_amd.ncf_head import _masks_as
    from pmgt_amd.ncf_model import ITEM_GMF, OUT_B, OUT_W, USER_GMF, _mlp_forward, ncf_model_shape, reads_gmf, reads_mlp
    from pmgt_amd.pair_train import head_weights
    w = head_weights(w, np.float64)
    _, layers, kind, ln = ncf_model_shape(w, kind)
    u, i = np.asarray(users[:1]), np.asarray(items[:1])
    m = {k: v[:1] for k, v in _masks_as(masks, np.float64).items()}
    feats = []
    if reads_gmf(kind):
        g = w[USER_GMF][u] * w[ITEM_GMF][i]
        feats.append(g * m["gmf"] if "gmf" in m else g)
    if reads_mlp(kind):
        feats.append(_mlp_forward(w, u, i, layers, ln, EPS, m)[0][-1])
    terms = np.concatenate(feats, axis=1)[0] * w[OUT_W].reshape(-1)
    return float(abs(terms.sum() + w[OUT_B][0]) / (np.abs(terms).sum() + abs(w[OUT_B][0])))


@functools.lru_cache(maxsize=None)
def world(shape, user_num=USER_NUM, item_num=ITEM_NUM, n=NS[-1], seed=None, drops=()):
    """The model, the pair list (duplicates forced; the last user and the last item never appear) and its labels, well-conditioned in eval
    mode and under every mask set of `drops` = ((p_emb, p_layer, step), ..)."""
    factor, layers, kind, ln = shape
    w = random_model(*shape, user_num, item_num, seed=5000 + 100 * factor + 10 * layers + len(kind))
    rng = np.random.default_rng((DROP_PAIR_SEEDS if drops else PAIR_SEEDS).get(shape, 29) if seed is None else seed)
    users, items = rng.integers(0, user_num - 1, size=n), rng.integers(0, item_num - 1, size=n)
    labels = (rng.random(n) < 0.4).astype(np.float32)
    redrawn = np.zeros(n, dtype=bool)
    for _ in range(64):
        bad = ill_conditioned(w, kind, users, items)
        for p_emb, p_layer, step in drops:
            bad |= ill_conditioned(w, kind, users, items, masks_of(shape, n, p_emb, list(p_layer) if isinstance(p_layer, tuple) else p_layer, step))
        bad = np.nonzero(bad)[0]
        if len(bad) == 0:
            break
        redrawn[bad] = True
        users[bad], items[bad] = rng.integers(0, user_num - 1, size=len(bad)), rng.integers(0, item_num - 1, size=len(bad))
    else:
        raise AssertionError(f"no well-conditioned pair list for {shape}")
    for m in (NS if n == NS[-1] else (n,)):
        assert redrawn[:m].sum() * 8 <= m, (shape, m, int(redrawn[:m].sum()))
    if n == NS[-1]:                                          # (the lists whose first pair is a case of its own)
        sets = [None] + [masks_of(shape, n, p_emb, list(p) if isinstance(p, tuple) else p, step) for p_emb, p, step in drops]
        worst = min(first_logit_condition(w, kind, users, items, ms) for ms in sets)
        assert worst >= FIRST_LOGIT, (shape, "the first pair's logit cancels", worst)
        for ms in sets:
            for m in NS:
                z = ncf_model_grad_host(w, users[:m], items[:m], labels[:m], np.float64, layer_norm_eps=EPS, kind=kind,
                                        masks=None if ms is None else cut(ms, m))[1]
                dl = 1 / (1 + np.exp(-z)) - labels[:m]
                assert abs(dl.sum()) >= FIRST_LOGIT * np.abs(dl).sum(), (shape, "the sum of the dlogits cancels", m, float(abs(dl.sum()) / np.abs(dl).sum()))
    return dict(shape=shape, kind=kind, w=w, users=users, items=items, labels=labels, redrawn=redrawn, user_num=user_num, item_num=item_num)


# the dropout cases of the GPU test: (p_emb, p of the layers): p = 0.2 everywhere; per-layer p's, one of them 0
DROPS = ((0.2, 0.2), (0.3, (0.1, 0.5, 0.0, 0.4)))
DROP_HEADS = [(8, 2, "NeuMF-end", True), (16, 3, "MLP", True), (32, 4, "MLP", True), (8, 2, "GMF", False)]
DROP_STEPS = (0, 7)


def drop_sets(shape):
    return tuple((p_emb, p if np.isscalar(p) else tuple(p[:shape[1]]), step) for p_emb, p in DROPS for step in DROP_STEPS)


def drop_world(shape, sets=drop_sets):
    return world(shape, drops=sets(shape))


def label_sets(h, n):
    return (("mixed", h["labels"][:n]), ("zeros", np.zeros(n, np.float32)), ("ones", np.ones(n, np.float32)))


def torch_grad(w, shape, users, items, labels, dtype=torch.float32):
    """The second realisation: loss, logits and every gradient by torch autograd through pmgt_amd.ncf.NCF on the CPU."""
    model = torch_model(w, shape, dtype).eval()
    logits = model((torch.from_numpy(users), torch.from_numpy(items)))
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, torch.from_numpy(labels).to(dtype))
    loss.backward()
    named = dict(model.named_parameters())
    out = {k: named[k].grad.numpy() for k in w}
    out.update(loss=np.asarray([loss.item()]), logits=logits.detach().numpy())
    return out


def torch_grad_masked(w, shape, users, items, labels, masks, dtype=torch.float32):
    """torch_grad in TRAINING-mode arithmetic under `masks`: every Dropout of the NCF multiplies by the mask of its site (forward hooks;
    emb_dropout is called on the GMF product first, then on the concatenated input: the reference's order)."""
    model = torch_model(w, shape, dtype).eval()
    as_t = {k: torch.from_numpy(np.asarray(keep)).to(dtype) * torch.tensor(float(scale), dtype=torch.float32).to(dtype) for k, (keep, scale) in masks.items()}
    order, calls = [s for s in ("gmf", "emb") if s in as_t], []
    model.emb_dropout.register_forward_hook(lambda mod, inp, out: (calls.append(1), out * as_t[order[len(calls) - 1]])[1])
    if shape[2] != "GMF":
        for i, m in enumerate(m for m in model.MLP_layers if isinstance(m, torch.nn.Dropout)):
            m.register_forward_hook(lambda mod, inp, out, i=i: out * as_t[f"layer{i}"])
    logits = model((torch.from_numpy(users), torch.from_numpy(items)))
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, torch.from_numpy(labels).to(dtype))
    loss.backward()
    named = dict(model.named_parameters())
    out = {k: named[k].grad.numpy() for k in w}
    out.update(loss=np.asarray([loss.item()]), logits=logits.detach().numpy())
    return out


def second_realisation_masked(shape, h):
    """torch autograd in fp32 under the masks on every case of the dropout GPU test -> the largest ratio of any quantity"""
    from tests.dcn_util import ratios
    worst = 0.0
    for p_emb, p, step in drop_sets(shape):
        full = masks_of(shape, NS[-1], p_emb, list(p) if isinstance(p, tuple) else p, step)
        for n in NS:
            users, items, labels, masks = h["users"][:n], h["items"][:n], h["labels"][:n], cut(full, n)
            o64, r32 = (host(h["w"], h["kind"], users, items, labels, dt, True, masks) for dt in (np.float64, np.float32))
            worst = max(worst, max(ratios(torch_grad_masked(h["w"], shape, users, items, labels, masks), o64, r32).values()))
    return worst


def permuted_host(w, shape, users, items, labels, masks=None, dtype=np.float32, seed=1):
    """A realisation of the yardstick in ANOTHER ORDER OF SUMS: ncf_model_grad_host on the model with the columns of every embedding table
    and the units of every layer permuted (the same function: the LayerNorm does not see the order of its row), the masks permuted with
    them and the gradients permuted back."""
    from pmgt_amd.ncf_model import ITEM_GMF, ITEM_MLP, OUT_W, USER_GMF, USER_MLP, layer_keys, reads_gmf, reads_mlp
    factor, layers, kind, ln = shape
    rng = np.random.default_rng(seed)
    v, back, m = {k: np.asarray(a) for k, a in w.items()}, {}, None if masks is None else dict(masks)

    def cols(key, perm, lo=0):
        a = v[key].copy()
        a[..., lo: lo + len(perm)] = a[..., lo: lo + len(perm)][..., perm]
        v[key] = a
        back.setdefault(key, []).append((-1, lo, np.argsort(perm)))

    def rows(key, perm):
        v[key] = v[key][perm]
        back.setdefault(key, []).append((0, 0, np.argsort(perm)))

    def mask_cols(site, perm, lo=0):
        if m is not None and site in m:
            keep = np.array(m[site][0])
            keep[:, lo: lo + len(perm)] = keep[:, lo: lo + len(perm)][:, perm]
            m[site] = (keep, m[site][1])

    at = 0
    if reads_gmf(kind):
        pg = rng.permutation(factor)
        cols(USER_GMF, pg), cols(ITEM_GMF, pg), cols(OUT_W, pg), mask_cols("gmf", pg)
        at = factor
    if reads_mlp(kind):
        d = factor << (layers - 1)
        pu, pi = rng.permutation(d), rng.permutation(d)
        first = layer_keys(0, ln)[0]
        cols(USER_MLP, pu), cols(ITEM_MLP, pi), cols(first, pu), cols(first, pi, d), mask_cols("emb", pu), mask_cols("emb", pi, d)
        for i in range(layers):
            perm = rng.permutation(d >> i)
            for key in layer_keys(i, ln):
                rows(key, perm)
            mask_cols(f"layer{i}", perm)
            cols(layer_keys(i + 1, ln)[0], perm) if i + 1 < layers else cols(OUT_W, perm, at)
    out = host(v, kind, users, items, labels, dtype, True, m)
    for key, moves in back.items():
        g = out[key]
        for axis, lo, inv in reversed(moves):
            if axis == 0:
                g = g[inv]
            else:
                g = g.copy()
                g[..., lo: lo + len(inv)] = g[..., lo: lo + len(inv)][..., inv]
        out[key] = g
    return out


PERMUTATIONS = (1, 2, 3)                                     # the seeds of permuted_host's permutations


def other_orders(shape, h, masked: bool):
    """permuted_host in fp32 under PERMUTATIONS on every case of the GPU test (masked: the dropout test's) -> (the largest ratio of any
    quantity, where)"""
    from tests.dcn_util import ratios
    kind, worst, where = h["kind"], 0.0, None
    sets = [(p_emb, list(p) if isinstance(p, tuple) else p, step) for p_emb, p, step in drop_sets(shape)] if masked else [None]
    for ds in sets:
        full = None if ds is None else masks_of(shape, NS[-1], *ds)
        for n in NS:
            for name, labels in (label_sets(h, n) if ds is None else (("mixed", h["labels"][:n]),)):
                users, items, masks = h["users"][:n], h["items"][:n], None if ds is None else cut(full, n)
                o64, r32 = (host(h["w"], kind, users, items, labels, dt, True, masks) for dt in (np.float64, np.float32))
                for ps in PERMUTATIONS:
                    rt = ratios(permuted_host(h["w"], shape, users, items, labels, masks, np.float32, ps), o64, r32)
                    k = max(rt, key=rt.get)
                    if rt[k] > worst:
                        worst, where = rt[k], (ds, n, name, k, ps)
    return worst, where


def abs_grad(w, kind, users, items, labels):
    """ncf_model_grad_host's backward in fp64 with every product and sum taken over absolute values -> {quantity: the magnitude of each
    element before cancellation} (the loss: sum_p |terms| / n): the measure of an in-order fp32 sum over the pairs."""
    from pmgt_amd.ncf_model import (ITEM_GMF, ITEM_MLP, OUT_B, OUT_W, USER_GMF, USER_MLP, _mlp_forward, layer_keys, ncf_model_shape, reads_gmf,
                                    reads_mlp)
    from pmgt_amd.pair_train import head_weights
    from tests.dcn_util import _ln_bwd_abs
    w = head_weights(w, np.float64)
    factor, layers, kind, ln = ncf_model_shape(w, kind)
    users, items, y = np.asarray(users), np.asarray(items), np.asarray(labels, dtype=np.float64)
    n = len(users)
    _, z, _ = ncf_model_grad_host(w, users, items, labels, np.float64, layer_norm_eps=EPS, kind=kind)
    e = np.exp(-np.abs(z))
    out = {"loss": np.asarray([(np.maximum(z, 0) + np.abs(z * y) + np.log1p(e)).sum() / n])}
    dl = np.abs((np.where(z >= 0, 1 / (1 + e), e / (1 + e)) - y) / n)
    feats = []
    if reads_gmf(kind):
        gu, gi = np.abs(w[USER_GMF][users]), np.abs(w[ITEM_GMF][items])
        feats.append(gu * gi)
    if reads_mlp(kind):
        hs, stats, _ = _mlp_forward(w, users, items, layers, ln, EPS, {})
        feats.append(np.abs(hs[-1]))
    feat = np.concatenate(feats, axis=1)
    wp = np.abs(w[OUT_W].reshape(-1))
    out[OUT_W], out[OUT_B] = (dl @ feat).reshape(1, -1), np.asarray([dl.sum()])
    dfeat = dl[:, None] * wp[None, :]
    if reads_gmf(kind):
        out[USER_GMF], out[ITEM_GMF] = np.zeros_like(w[USER_GMF]), np.zeros_like(w[ITEM_GMF])
        np.add.at(out[USER_GMF], users, dfeat[:, :factor] * gi)
        np.add.at(out[ITEM_GMF], items, dfeat[:, :factor] * gu)
    if reads_mlp(kind):
        dh = dfeat[:, factor:] if reads_gmf(kind) else dfeat
        for i in reversed(range(layers)):
            keys = layer_keys(i, ln)
            da = dh * (hs[i + 1] > 0)
            if ln:
                xhat, rstd = stats[i]
                out[keys[2]], out[keys[3]] = (da * np.abs(xhat)).sum(axis=0), da.sum(axis=0)
                da = _ln_bwd_abs(da, w[keys[2]], xhat, rstd)
            out[keys[0]], out[keys[1]] = da.T @ np.abs(hs[i]), da.sum(axis=0)
            dh = da @ np.abs(w[keys[0]])
        d = w[USER_MLP].shape[1]
        out[USER_MLP], out[ITEM_MLP] = np.zeros_like(w[USER_MLP]), np.zeros_like(w[ITEM_MLP])
        np.add.at(out[USER_MLP], users, dh[:, :d])
        np.add.at(out[ITEM_MLP], items, dh[:, d:])
    return out


def _second_realisations(shape, h, masked: bool) -> float:
    if masked:
        return max(second_realisation_masked(shape, h), other_orders(shape, h, True)[0])
    from tests.dcn_util import ratios
    worst = other_orders(shape, h, False)[0]
    for n in NS:
        for _, labels in label_sets(h, n):
            users, items = h["users"][:n], h["items"][:n]
            o64, r32 = (host(h["w"], h["kind"], users, items, labels, dt) for dt in (np.float64, np.float32))
            worst = max(worst, max(ratios(torch_grad(h["w"], shape, users, items, labels), o64, r32).values()))
    return worst


if __name__ == "__main__":                                   # the choice of PAIR_SEEDS and DROP_PAIR_SEEDS
    for name, shapes, masked in (("PAIR_SEEDS", HEADS + OTHER_HEADS, False), ("DROP_PAIR_SEEDS", DROP_HEADS, True)):
        found = {}
        for shape in shapes:
            for seed in range(29, 229):
                try:
                    h = world(shape, seed=seed, drops=drop_sets(shape) if masked else ())
                except AssertionError as e:
                    print(name, shape, "seed", seed, "refused:", e.args[0][1:] if isinstance(e.args[0], tuple) else e)
                    continue
                worst = _second_realisations(shape, h, masked) if shape not in OTHER_HEADS else 0.0
                print(name, shape, "seed", seed, f"the other realisations: largest ratio {worst:.2f}")
                if worst <= 4.0:
                    found[shape] = seed
                    break
        print(name, "=", found)
