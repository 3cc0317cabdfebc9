"""Shared by the DCN tests: seeded models, the two host realisations of the yardstick (numpy: pmgt_amd.dcn_head; torch autograd through
pmgt_amd.dcn.DCN), the project's measure with the floor of the DEGENERATE tensors, and the choice of well-conditioned pairs.

THE MEASURE, per quantity (loss, logits, each gradient tensor), o64 / r32 = dcn_head_grad_host in fp64 / fp32:
    max|x - o64| <= C max(max|r32 - o64|, 2^-22 max|o64|),   C = 4, the project's factor.
DEGENERATE TENSORS.  With LayerNorm and dropout 0, LN(x0 (1 + s)) does not depend on |1 + s|, so d loss / d cross_net.layers.c.weight, and
d loss / d (gamma, beta) of every cross layer but the last, are 0 in exact arithmetic: o64 is ~1e-10 or below and r32 is rounding noise,
whose size depends on the order of the sums.  For them the floor 2^-22 max|o64| is replaced by FLOOR_FACTOR 2^-22 M, M = the largest element
of the ABSOLUTE-VALUE BACKWARD pass (abs_grad: the same backward with every product and sum taken over absolute values, the LayerNorm
backward bounded by rstd (|g'| + mean|g'| + |xhat| mean|g' xhat|)): the magnitude before cancellation.  FLOOR_FACTOR is settled on the
CPU by a second fp32 realisation, torch autograd (tests/test_dcn_measure_cpu.py), never by the code under test.

WELL-CONDITIONED PAIRS, chosen on the host before the device computes anything: a pair is drawn again when
    a pre-ReLU value of its row lies within 8 x the fp32-numpy error of its layer from 0           (the ReLU is discontinuous there), or
    some |1 + s_c| < 2^-10 (1 + sum_j |x_j^(c) w_cj|)                                           (LN(x0 (1 + s)) changes sign there);
at most 1 pair in 8 of a case may be drawn again (world() asserts it for every n of NS)."""
import functools

import numpy as np
import torch

from pmgt_amd.dcn_head import ITEM_KEY, OUT_B, OUT_W, USER_KEY, _forward, dcn_head_grad_host, dcn_layout, head_weights

HEADS = [(8, 1, 1, False), (8, 2, 3, True), (16, 1, 4, True), (32, 3, 3, True), (64, 1, 6, False), (16, 4, 2, True)]
NS = (1, 31, 33, 130)
USER_NUM, ITEM_NUM = 5, 7
C_BOUND = 4.0
FLOOR_FACTOR = 1.0      # of the degenerate tensors' floor: see tests/test_dcn_measure_cpu.py
EPS = 1e-12
# the pair lists: seeds for which the yardstick alone draws at most 1 pair in 8 again, for every n of NS (checked on the CPU)
PAIR_SEEDS = {h: 29 for h in HEADS}


def head_id(h):
    return f"f{h[0]}-L{h[1]}-C{h[2]}-{'ln' if h[3] else 'noln'}"


def random_dcn(factor, deep, cross, ln, user_num, item_num, seed):
    """The trained tensors of a DCN as fp32 numpy arrays keyed like the state_dict, every one away from its init's special values
    (gamma != 1, beta != 0, biases != 0), scaled so that the logits stay O(1) with and without LayerNorm.  With LayerNorm the cross weights
    are 0.3 / sqrt(D) in size: s_c = x^(c) . w_c is then about N(0, 0.1), 1 + s_c stays away from 0 and LN_c's rstd = 1 / (|1 + s_c|
    std(x0)) stays O(1).  The reason is the DEGENERATE path: d s_c is an exactly cancelling sum, so it is rounding noise, which
    d x^(c) = d s_c w_c hands down and every rstd below amplifies into the embedding gradients.  That leak is proportional to |w_c| rstd:
    with cross weights of size 1 / sqrt(D) (1 + s_c near 0 for some pair of every list, rstd up to 40) or of the reference's init scale
    U(-1, 1) it decided the embedding gradients' error of BOTH host realisations, which then differed from each other by up to 13 x and
    4.2 x on single cases of head (32, 3, 3, on): a property of those weights, not of any realisation."""
    rng = np.random.default_rng(seed)
    layout, _ = dcn_layout(factor, deep, cross, ln, user_num, item_num)
    D = 2 * (factor << deep)
    w = {}
    for key, (_, shape) in layout.items():
        v = rng.standard_normal(shape)
        if key in (USER_KEY, ITEM_KEY):
            v *= 1.0 if ln else 0.5
        elif key.endswith("linear.weight") or key == OUT_W:
            v *= 1.0 / np.sqrt(shape[1])
        elif key.endswith("layer_norm.weight"):
            v = 1.0 + 0.3 * v
        elif key.endswith("bias"):
            v *= 0.3
        else:                                                # the cross weights [D, 1]
            v *= (0.3 if ln else 1.0) / np.sqrt(D)
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


def host(w, users, items, labels, dtype):
    loss, logits, grads = dcn_head_grad_host(w, users, items, labels, dtype, layer_norm_eps=EPS)
    return dict(grads, loss=np.asarray([loss]), logits=logits)


def torch_model(w, shape, dtype=torch.float32, device="cpu"):
    """A pmgt_amd.dcn.DCN holding `w`."""
    from pmgt_amd.dcn import DCN
    factor, deep, cross, ln = shape
    model = DCN(len(w[USER_KEY]), len(w[ITEM_KEY]), factor, deep, cross, use_layer_norm=ln, layer_norm_eps=EPS).to(dtype)
    missing = model.load_state_dict({k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in w.items()}, strict=False)
    assert not missing.unexpected_keys and all(k.startswith("cross_net") and k.endswith(".bias") and "layer_norm" not in k
                                               for k in missing.missing_keys)
    return model.to(device).eval()


def torch_grad(w, shape, users, items, labels, dtype=torch.float32):
    """The second realisation: loss, logits and every gradient by torch autograd through pmgt_amd.dcn.DCN on the CPU."""
    model = torch_model(w, shape, dtype)
    logits = model((torch.from_numpy(users), torch.from_numpy(items)))
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, torch.from_numpy(labels).to(dtype))
    loss.backward()
    named = dict(model.named_parameters())
    out = {k: named[k].grad.numpy() for k in w}
    out.update(loss=np.asarray([loss.item()]), logits=logits.detach().numpy())
    return out


def degenerate_keys(shape):
    factor, deep, cross, ln = shape
    if not ln:
        return []
    keys = [f"cross_net.layers.{c}.weight" for c in range(cross)]
    for c in range(cross - 1):
        keys += [f"cross_net.layers.{c}.layer_norm.weight", f"cross_net.layers.{c}.layer_norm.bias"]
    return keys


def _ln_bwd_abs(g, gamma, xhat, rstd):
    gp = g * np.abs(gamma)
    return rstd * (gp + gp.mean(axis=1, keepdims=True) + np.abs(xhat) * (gp * np.abs(xhat)).mean(axis=1, keepdims=True))


def abs_grad(w, users, items, labels):
    """dcn_head_grad_host's backward in fp64 with every product and sum taken over absolute values -> {quantity: the magnitude of each
    element before cancellation} (the loss: sum_p |terms| / n).  Also the measure of an in-order fp32 sum over the pairs."""
    w = head_weights(w, np.float64)
    L = sum(1 for k in w if k.endswith("linear.weight"))
    C = sum(1 for k in w if k.startswith("cross_net") and k.endswith(".weight") and "layer_norm" not in k)
    ln = "deep_net.layers.0.layer_norm.weight" in w
    users, items, y = np.asarray(users), np.asarray(items), np.asarray(labels, dtype=np.float64)
    n = len(users)
    x0, xs, cross, hs, deep, feat, z = _forward(w, users, items, EPS)
    D = x0.shape[1]
    e = np.exp(-np.abs(z))
    out = {"loss": np.asarray([(np.maximum(z, 0) + np.abs(z * y) + np.log1p(e)).sum() / n])}
    dl = np.abs((np.where(z >= 0, 1 / (1 + e), e / (1 + e)) - y) / n)
    wo = np.abs(w[OUT_W].reshape(-1))
    out[OUT_W], out[OUT_B] = (dl @ np.abs(feat)).reshape(1, -1), np.asarray([dl.sum()])
    dfeat = dl[:, None] * wo[None, :]
    g, dx0, ax0 = dfeat[:, :D], np.zeros_like(x0), np.abs(x0)
    for c in reversed(range(C)):
        s, xhat, rstd = cross[c]
        p = f"cross_net.layers.{c}."
        if ln:
            out[p + "layer_norm.weight"], out[p + "layer_norm.bias"] = (g * np.abs(xhat)).sum(axis=0), g.sum(axis=0)
            g = _ln_bwd_abs(g, w[p + "layer_norm.weight"], xhat, rstd)
        ds = (g * ax0).sum(axis=1)
        dx0 = dx0 + g * np.abs(s)[:, None] + g
        out[p + "weight"] = (ds @ np.abs(xs[c])).reshape(-1, 1)
        g = ds[:, None] * np.abs(w[p + "weight"].reshape(-1))[None, :]
    dx0 = dx0 + g
    dh = dfeat[:, D:]
    for l in reversed(range(L)):
        a, xhat, rstd = deep[l]
        p = f"deep_net.layers.{l}."
        da = dh * (hs[l + 1] > 0)
        if ln:
            out[p + "layer_norm.weight"], out[p + "layer_norm.bias"] = (da * np.abs(xhat)).sum(axis=0), da.sum(axis=0)
            da = _ln_bwd_abs(da, w[p + "layer_norm.weight"], xhat, rstd)
        out[p + "linear.weight"], out[p + "linear.bias"] = da.T @ np.abs(hs[l]), da.sum(axis=0)
        dh = da @ np.abs(w[p + "linear.weight"])
    dx0 = dx0 + dh
    E = D // 2
    out[USER_KEY], out[ITEM_KEY] = np.zeros_like(w[USER_KEY]), np.zeros_like(w[ITEM_KEY])
    np.add.at(out[USER_KEY], users, dx0[:, :E])
    np.add.at(out[ITEM_KEY], items, dx0[:, E:])
    return out


def ratios(got, o64, r32, shape=None, magnitudes=None, floor_factor=FLOOR_FACTOR):
    """{quantity: max|got - o64| / max(max|r32 - o64|, floor)}; floor = 2^-22 max|o64|, for the degenerate tensors of `shape`
    floor_factor 2^-22 max(magnitudes[quantity])"""
    degenerate = degenerate_keys(shape) if shape is not None else []
    out = {}
    for k in o64:
        ref = np.asarray(o64[k], dtype=np.float64)
        floor = floor_factor * 2.0 ** -22 * np.abs(magnitudes[k]).max() if k in degenerate else 2.0 ** -22 * np.abs(ref).max()
        scale = max(np.abs(np.asarray(r32[k], dtype=np.float64) - ref).max(), floor)
        err = np.abs(np.asarray(got[k], dtype=np.float64).reshape(ref.shape) - ref).max()
        out[k] = err / scale if scale > 0 else (0.0 if err == 0 else np.inf)
    return out


def ill_conditioned(w, users, items):
    """bool [n]: the pairs the header's two rules draw again"""
    w64, w32 = head_weights(w, np.float64), head_weights(w, np.float32)
    f64, f32 = _forward(w64, users, items, EPS), _forward(w32, users, items, EPS)
    bad = np.zeros(len(users), dtype=bool)
    for (a64, _, _), (a32, _, _) in zip(f64[4], f32[4]):      # the pre-ReLU values of every deep layer
        bad |= ~(np.abs(a64).min(axis=1) > 8 * np.abs(a32 - a64).max())
    xs, cross = f64[1], f64[2]
    for c, (s, _, _) in enumerate(cross):
        wc = w64[f"cross_net.layers.{c}.weight"].reshape(-1)
        bad |= np.abs(1 + s) < 2.0 ** -10 * (1 + (np.abs(xs[c]) * np.abs(wc)[None, :]).sum(axis=1))
    return bad


@functools.lru_cache(maxsize=None)
def world(shape, user_num=USER_NUM, item_num=ITEM_NUM, n=NS[-1], seed=None):
    """The model, the pair list (duplicates forced; the last user and the last item never appear) and its labels, well-conditioned."""
    factor, deep, cross, ln = shape
    w = random_dcn(*shape, user_num, item_num, seed=4000 + 100 * factor + 10 * deep + cross)
    layout, count = dcn_layout(*shape, user_num, item_num)
    rng = np.random.default_rng(PAIR_SEEDS.get(shape, 29) if seed is None else seed)
    users, items = rng.integers(0, user_num - 1, size=n), rng.integers(0, item_num - 1, size=n)
    labels = (rng.random(n) < 0.4).astype(np.float32)
    redrawn = np.zeros(n, dtype=bool)
    for _ in range(64):
        bad = np.nonzero(ill_conditioned(w, users, items))[0]
        if len(bad) == 0:
            break
        redrawn[bad] = True
        users[bad], items[bad] = rng.integers(0, user_num - 1, size=len(bad)), rng.integers(0, item_num - 1, size=len(bad))
    else:
        raise AssertionError(f"no well-conditioned pair list for {shape}")
    for m in (NS if n == NS[-1] else (n,)):
        assert redrawn[:m].sum() * 8 <= m, (shape, m, int(redrawn[:m].sum()))
    return dict(shape=shape, w=w, layout=layout, count=count, users=users, items=items, labels=labels, redrawn=redrawn,
                user_num=user_num, item_num=item_num)


def label_sets(h, n):
    return (("mixed", h["labels"][:n]), ("zeros", np.zeros(n, np.float32)), ("ones", np.ones(n, np.float32)))
