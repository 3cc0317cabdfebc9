"""Shared by the DCN dropout tests: the mask sets, the host realisations of the masked yardstick (numpy: dcn_head_grad_host(masks=);
torch autograd through pmgt_amd.dcn.DCN with its Dropout modules replaced by stubs that multiply by the given masks), tests/dcn_util.py's
measure with the p-DEPENDENT degenerate set, and the choice of well-conditioned pairs under every mask set.

THE MEASURE is dcn_util's, C = 4, FLOOR_FACTOR = 1:  max|x - o64| <= 4 max(max|r32 - o64|, floor),  o64 / r32 =
dcn_head_grad_host(masks=...) in fp64 / fp32, floor = 2^-22 max|o64|, for a degenerate tensor 2^-22 M with M from the absolute-value
backward UNDER THE MASKS (abs_grad_masked: a mask is a non-negative factor, so it multiplies the magnitudes as it multiplies the values).
DEGENERATE TENSORS with LayerNorm (degenerate_keys_p): cross layer c's w_c unless its own mask is drawn (p_cross[c] > 0: then x0 (m s + 1)
is no multiple of x0) AND x^(c+1) still has a gradient; gamma and beta of cross layer c < C - 1 unless x^(c+1) has one, which it has
when every layer above c draws a mask (x^(c+1) is read through s_(c+1) alone).  With one p_cross for every layer, as in every mask set
of the tests: none when it is > 0; with emb_dropout alone the set is dcn_util.degenerate_keys'.
NEARLY DEGENERATE TENSORS.  A tensor of dcn_util.degenerate_keys that the cross masks bring to life is the small remainder of the same
cancelling sums (ds_c = sum_j g_j m_cj x0_j with sum_j g_j u_j = 0 exactly: |value| 1e-4 .. 1e-2 where the terms are O(1)), so its fp32
error is a few 2^-24 of the TERMS, 10 to 100 x 2^-24 of the value, and differs between any two realisations by more than C: with the
plain floor the SECOND fp32 realisation (torch autograd under the stub masks, on the CPU) misses the bound on these tensors at nearly
every pair list (ratios 4 to 18 over the seeds 29 .. 40 of the five LayerNorm models, 38 at most over 29 .. 79).  Their floor is
therefore NEAR_FLOOR_FACTOR 2^-22 max|o64| with NEAR_FLOOR_FACTOR = 16, the smallest power of two at which that realisation passes
with a factor 2 to spare (tests/test_dcn_dropout_cpu.py asserts it); settled on the CPU, never by the code under test.  The bound on such
a tensor is then 4 x 16 x 2^-22 = 1.5e-5 of its largest element: a wrong keep decision, a mask at another (row, column) or a missing
1 / (1 - p) misses it by orders of magnitude.  FLOOR_FACTOR of the degenerate tensors stays 1.

WELL-CONDITIONED PAIRS.  dcn_util's two rules, evaluated under EVERY mask set of the test (PS x STEPS; a site's row is the pair's index, so
the rows of n = 130 are the rows of every smaller n), before the device computes anything: a pair is drawn again when
    a pre-ReLU value of its row lies within 8 x the fp32-numpy error of its layer from 0 (without LayerNorm the dropped elements, which are
    0 exactly in every realisation and pass no gradient, are left out), or
    |1 + s'| < 2^-10 (1 + sum_j |x_j^(c) w_cj| f) for (s', f) = (s_c, 1) and (s_c / (1 - p_c), 1 / (1 - p_c)): the two factors an element of
    x0 (m s_c + 1) carries.
At most 1 pair in 8 of a case may be drawn again.  PAIR_SEEDS: per model the first seed from 29 on at which this holds for every n of NS
AND the second fp32 realisation passes the measure on every case (a sum over the pairs such as output_layer.bias, or the one logit of
n = 1, can be small by cancellation too; a list on which a right realisation misses the bound cannot judge a kernel) -- both decided on
the CPU by the yardstick's realisations alone (python -m tests.dcn_dropout_util prints the search)."""
import functools

import numpy as np
import torch

from pmgt_amd.dcn_head import ITEM_KEY, OUT_B, OUT_W, USER_KEY, _forward, dcn_dropout_masks, dcn_head_grad_host, dcn_layout, head_weights
from tests.dcn_util import C_BOUND, EPS, HEADS, ITEM_NUM, NS, USER_NUM, _ln_bwd_abs, degenerate_keys, random_dcn, ratios, torch_model

SEED = 0x1234_5678_9ABC                                      # (above 2^32: both halves of the seed take part)
PS = [(0.2, 0.0, 0.0), (0.0, 0.5, 0.0), (0.0, 0.0, 0.5), (0.1, 0.3, 0.3)]      # (p_emb, p_deep, p_cross)
STEPS = (0, 7)
NEAR_FLOOR_FACTOR = 16.0                                     # of the nearly degenerate tensors' floor: see the header
# the pair lists (chosen on the CPU: python -m tests.dcn_dropout_util)
PAIR_SEEDS = {**{h: 29 for h in HEADS}, (32, 3, 3, True): 36, (64, 1, 6, False): 42}


def masks_of(shape, n, p, step, seed=SEED):
    return dcn_dropout_masks(seed, step, n, *shape[:3], *p)


def cut(masks, n):
    """the first n rows of every site"""
    return {k: (keep[:n], scale) for k, (keep, scale) in masks.items()}


def host_masked(w, users, items, labels, dtype, masks):
    loss, logits, grads = dcn_head_grad_host(w, users, items, labels, dtype, layer_norm_eps=EPS, masks=masks)
    return dict(grads, loss=np.asarray([loss]), logits=logits)


class MaskStub(torch.nn.Module):
    """What stands where a Dropout stood: a multiplication by a given mask"""

    def __init__(self, keep, scale, dtype, p):
        super().__init__()
        self.mask = torch.from_numpy(np.asarray(keep)).to(dtype) * torch.tensor(float(scale), dtype=torch.float32).to(dtype)
        self.p = p

    def forward(self, x):
        return x * self.mask


def set_stubs(model, masks, dtype=torch.float32):
    """every Dropout (or earlier stub) of a dcn.DCN replaced by the stub of its site under `masks`"""
    model.emb_dropout = MaskStub(*masks["emb"], dtype, model.emb_dropout.p)
    for l, layer in enumerate(model.deep_net.layers):
        layer.dropout = MaskStub(*masks[f"deep{l}"], dtype, layer.dropout.p)
    for c, layer in enumerate(model.cross_net.layers):
        layer.dropout = MaskStub(*masks[f"cross{c}"], dtype, layer.dropout.p)
    return model


def stub_model(w, shape, masks, dtype=torch.float32):
    """pmgt_amd.dcn.DCN holding `w`, every Dropout replaced by the stub of its site"""
    return set_stubs(torch_model(w, shape, dtype), masks, dtype)


def set_dropout(model, p_emb, p):
    """the p of every Dropout of a dcn.DCN, as its constructor's emb_dropout and dropout would set them"""
    model.emb_dropout.p = p_emb
    model.dropout_p = p
    for layer in list(model.deep_net.layers) + list(model.cross_net.layers):
        layer.dropout.p = p
    return model


def torch_grad_masked(w, shape, users, items, labels, masks, dtype=torch.float32):
    """Loss, logits and every gradient by torch autograd through dcn.DCN itself under the stub masks."""
    model = stub_model(w, shape, masks, dtype)
    logits = model((torch.from_numpy(users), torch.from_numpy(items)))
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, torch.from_numpy(labels).to(dtype))
    loss.backward()
    named = dict(model.named_parameters())
    out = {k: named[k].grad.numpy() for k in w}
    out.update(loss=np.asarray([loss.item()]), logits=logits.detach().numpy())
    return out


def degenerate_keys_p(shape, p_cross):
    """The tensors whose gradient is 0 in exact arithmetic: x^(c+1) is read through s_(c+1) alone (c + 1 < C), and LN(x0 (1 + s)) does not
    depend on s unless the layer's own mask is drawn; so d loss / d x^(c+1) is LIVE when every layer above c draws a mask, w_c has a
    gradient when its own mask is drawn and x^(c+1) is live, gamma and beta of layer c when x^(c+1) is live.  With one p for every layer:
    none when p > 0, dcn_util.degenerate_keys' when p = 0."""
    factor, deep, cross, ln = shape
    if not ln:
        return []
    p_cross = [p_cross] * cross if np.isscalar(p_cross) else list(p_cross)
    live = [all(p > 0 for p in p_cross[c + 1:]) for c in range(cross)]      # of x^(c+1); the last is read by the output layer
    keys = [f"cross_net.layers.{c}.weight" for c in range(cross) if not (p_cross[c] > 0 and live[c])]
    for c in range(cross):
        if not live[c]:
            keys += [f"cross_net.layers.{c}.layer_norm.weight", f"cross_net.layers.{c}.layer_norm.bias"]
    return keys


def abs_grad_masked(w, users, items, labels, masks):
    """dcn_util.abs_grad under `masks`: dcn_head_grad_host's masked backward in fp64 with every product and sum over absolute values."""
    w = head_weights(w, np.float64)
    L = sum(1 for k in w if k.endswith("linear.weight"))
    C = sum(1 for k in w if k.startswith("cross_net") and k.endswith(".weight") and "layer_norm" not in k)
    ln = "deep_net.layers.0.layer_norm.weight" in w
    m = {k: keep.astype(np.float64) * np.float64(scale) for k, (keep, scale) in masks.items()}
    users, items, y = np.asarray(users), np.asarray(items), np.asarray(labels, dtype=np.float64)
    n = len(users)
    x0, xs, cross, hs, deep, feat, z = _forward(w, users, items, EPS, masks)
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
        gm = g * m[f"cross{c}"]
        ds = (gm * ax0).sum(axis=1)
        dx0 = dx0 + gm * np.abs(s)[:, None] + g
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
        da = da * m[f"deep{l}"]
        out[p + "linear.weight"], out[p + "linear.bias"] = da.T @ np.abs(hs[l]), da.sum(axis=0)
        dh = da @ np.abs(w[p + "linear.weight"])
    dx0 = (dx0 + dh) * m["emb"]
    E = D // 2
    out[USER_KEY], out[ITEM_KEY] = np.zeros_like(w[USER_KEY]), np.zeros_like(w[ITEM_KEY])
    np.add.at(out[USER_KEY], users, dx0[:, :E])
    np.add.at(out[ITEM_KEY], items, dx0[:, E:])
    return out


def near_keys_p(shape, p_cross):
    """the nearly degenerate tensors: dcn_util.degenerate_keys that the cross masks bring to life"""
    dead = degenerate_keys_p(shape, p_cross)
    return [k for k in degenerate_keys(shape) if k not in dead]


def ratios_p(got, o64, r32, shape, p_cross, magnitudes):
    """dcn_util.ratios with the floors of the header: {quantity: max|got - o64| / max(max|r32 - o64|, floor)}"""
    out = ratios(got, o64, r32)                              # (the plain floor for every quantity)
    floors = {k: 2.0 ** -22 * np.abs(magnitudes[k]).max() for k in degenerate_keys_p(shape, p_cross)}      # FLOOR_FACTOR 1
    floors.update({k: NEAR_FLOOR_FACTOR * 2.0 ** -22 * np.abs(o64[k]).max() for k in near_keys_p(shape, p_cross)})
    for k, floor in floors.items():
        ref = np.asarray(o64[k], dtype=np.float64)
        scale = max(np.abs(np.asarray(r32[k], dtype=np.float64) - ref).max(), floor)
        out[k] = np.abs(np.asarray(got[k], dtype=np.float64).reshape(ref.shape) - ref).max() / scale
    return out


def second_realisation(shape, h):
    """torch autograd in fp32 under the stub masks on every case of the GPU test -> (the largest ratio of a nearly degenerate tensor, of
    any other quantity, the largest error / floor of a degenerate tensor of either realisation)"""
    near, rest, dead = 0.0, 0.0, 0.0
    for p in PS:
        for step in STEPS:
            full = masks_of(shape, NS[-1], p, step)
            for n in NS:
                users, items, labels, masks = h["users"][:n], h["items"][:n], h["labels"][:n], cut(full, n)
                o64, r32 = (host_masked(h["w"], users, items, labels, dt, masks) for dt in (np.float64, np.float32))
                t32 = torch_grad_masked(h["w"], shape, users, items, labels, masks)
                mags = abs_grad_masked(h["w"], users, items, labels, masks)
                assert sorted(t32) == sorted(o64) == sorted(list(mags) + ["logits"])
                for k, v in ratios_p(t32, o64, r32, shape, p[2], mags).items():
                    if k in near_keys_p(shape, p[2]):
                        near = max(near, v)
                    else:
                        rest = max(rest, v)
                for k in degenerate_keys_p(shape, p[2]):
                    floor = 2.0 ** -22 * np.abs(mags[k]).max()
                    assert np.abs(o64[k]).max() < floor, (k, "not degenerate")
                    dead = max(dead, np.abs(t32[k].reshape(o64[k].shape) - o64[k]).max() / floor, np.abs(r32[k] - o64[k]).max() / floor)
    return near, rest, dead


def ill_conditioned_masked(w, users, items, masks):
    """bool [n]: the pairs the header's two rules draw again under `masks`"""
    w64, w32 = head_weights(w, np.float64), head_weights(w, np.float32)
    ln = "deep_net.layers.0.layer_norm.weight" in w64
    f64, f32 = _forward(w64, users, items, EPS, masks), _forward(w32, users, items, EPS, masks)
    bad = np.zeros(len(users), dtype=bool)
    for l, ((a64, _, _), (a32, _, _)) in enumerate(zip(f64[4], f32[4])):      # the pre-ReLU values of every deep layer
        dist = np.abs(a64) if ln else np.where(masks[f"deep{l}"][0], np.abs(a64), np.inf)
        bad |= ~(dist.min(axis=1) > 8 * np.abs(a32 - a64).max())
    xs, cross = f64[1], f64[2]
    for c, (s, _, _) in enumerate(cross):
        wc = w64[f"cross_net.layers.{c}.weight"].reshape(-1)
        mag = (np.abs(xs[c]) * np.abs(wc)[None, :]).sum(axis=1)
        for f in (1.0, float(masks[f"cross{c}"][1])):
            bad |= np.abs(1 + s * f) < 2.0 ** -10 * (1 + mag * f)
    return bad


def ill_conditioned_any(shape, w, users, items):
    bad = np.zeros(len(users), dtype=bool)
    for p in PS:
        for step in STEPS:
            bad |= ill_conditioned_masked(w, users, items, masks_of(shape, len(users), p, step))
    return bad


@functools.lru_cache(maxsize=None)
def world(shape, user_num=USER_NUM, item_num=ITEM_NUM, n=NS[-1], seed=None):
    """dcn_util.world's model with a pair list (duplicates forced; the last user and the last item never appear) that is well-conditioned
    under every mask set of the test."""
    factor, deep, cross, ln = shape
    w = random_dcn(*shape, user_num, item_num, seed=4000 + 100 * factor + 10 * deep + cross)
    layout, count = dcn_layout(*shape, user_num, item_num)
    rng = np.random.default_rng(PAIR_SEEDS.get(shape, 29) if seed is None else seed)
    users, items = rng.integers(0, user_num - 1, size=n), rng.integers(0, item_num - 1, size=n)
    labels = (rng.random(n) < 0.4).astype(np.float32)
    redrawn = np.zeros(n, dtype=bool)
    for _ in range(64):
        bad = np.nonzero(ill_conditioned_any(shape, w, users, items))[0]
        if len(bad) == 0:
            break
        redrawn[bad] = True
        users[bad], items[bad] = rng.integers(0, user_num - 1, size=len(bad)), rng.integers(0, item_num - 1, size=len(bad))
    else:
        raise AssertionError(f"no well-conditioned pair list for {shape}")
    for m in NS:
        assert redrawn[:m].sum() * 8 <= m, (shape, m, int(redrawn[:m].sum()))
    return dict(shape=shape, w=w, layout=layout, count=count, users=users, items=items, labels=labels, redrawn=redrawn,
                user_num=user_num, item_num=item_num)


if __name__ == "__main__":                                   # the choice of PAIR_SEEDS
    for shape in HEADS:
        for seed in range(29, 129):
            try:
                h = world(shape, seed=seed)
            except AssertionError:
                print(shape, "seed", seed, "outside the cap")
                continue
            near, rest, dead = second_realisation(shape, h)
            print(shape, "seed", seed, "drawn again", [int(h["redrawn"][:m].sum()) for m in NS],
                  f"second realisation: nearly degenerate {near:.2f}, other quantities {rest:.2f}, degenerate error / floor {dead:.2f}")
            if near <= C_BOUND / 2 and rest <= C_BOUND and dead <= 2:
                break
