"""pmgt_ncf_train_grad on synthetic heads: loss, logits and every gradient tensor against ncf_head_grad_host in fp64, with the error of the
same formula in fp32 numpy as the measure.

Per case and per quantity (loss, logits, each gradient tensor), o64 = ncf_head_grad_host(..., np.float64), r32 = the same in np.float32:
    max|kernel - o64| <= C max(max|r32 - o64|, 2^-22 max|o64|),   C = 4, the project's factor (tests/test_ncf_score_gpu.py).
The kernel and r32 round the same fp32 operations and differ by the order of their sums only (MFMA k-order, the 16 | 16 split of a
32-chunk, four accumulators over the pairs), so the error classes are the same; a bf16 operand, a dropped ReLU mask or a lost duplicate row
misses by orders of magnitude.  user_num = 5 and I = 7 with pairs drawn from 4 users x 6 items: duplicates are forced, user 4 and item 6
never appear and their gradient rows must be exactly +0.0.
Measured on the MI355X (one run): the largest ratio of any quantity per head 2.25, 1.52, 2.01, 2.95, 2.61, 2.90; saturated logits at most 2.00.

The largest case the entry takes (65 536 pairs) runs once on a small head: there the weight gradients are sums of 16 384 terms per
accumulator, which BLAS (r32) blocks and the kernel adds in order, so they are judged by the bound of an in-order fp32 sum,
(n / 4 + 3 + 64) 2^-24 sum_p |dz_p| |x_p| per element (n / 4 terms per accumulator, the tree of four, 64 for the roundings inside a
term), everything else by the bound above."""
import ctypes as C

import numpy as np
import pytest
import torch

from pmgt_amd.ncf_train import NcfHeadGrad, NcfTrainC, head_layout, ncf_head_grad_host
from tests.test_recommend_cpu import random_head

pytestmark = pytest.mark.gpu

HEADS = [(8, 1, "MLP"), (8, 2, "NeuMF-end"), (16, 3, "MLP"), (64, 2, "NeuMF-end"), (64, 3, "NeuMF-end"), (32, 4, "MLP")]
NS = (1, 31, 33, 130)
USER_NUM, ITEM_NUM = 5, 7
C_BOUND = 4.0


def flatten(w, layout, count):
    flat = np.zeros(count, dtype=np.float32)
    for key, (off, shape) in layout.items():
        flat[off: off + w[key].size] = w[key].reshape(-1)
    return flat


def device_grad(w, table, shape, user_num):
    layout, count = head_layout(*shape, user_num, len(table))
    params = torch.from_numpy(flatten(w, layout, count)).cuda()
    grads = torch.full((count,), float("nan"), device="cuda")
    return NcfHeadGrad(*shape, user_num, torch.from_numpy(table).cuda(), params, grads), layout


def run(fn, users, items, labels):
    fn.grads.fill_(float("nan"))                             # the buffer is written whole: no NaN may survive
    loss, logits = fn(torch.from_numpy(users).cuda(), torch.from_numpy(items).cuda(), torch.from_numpy(labels).cuda())
    return loss.clone(), logits.clone(), fn.grads.clone()


def ratios(got, o64, r32):
    """{quantity: max|got - o64| / max(max|r32 - o64|, 2^-22 max|o64|)}"""
    out = {}
    for k in o64:
        ref = np.asarray(o64[k], dtype=np.float64)
        scale = max(np.abs(np.asarray(r32[k], dtype=np.float64) - ref).max(), 2.0 ** -22 * np.abs(ref).max())
        err = np.abs(np.asarray(got[k], dtype=np.float64) - ref).max()
        out[k] = err / scale if scale > 0 else (0.0 if err == 0 else np.inf)
    return out


def split(loss, logits, grads, layout):
    g = grads.cpu().numpy()
    out = {"loss": loss.cpu().numpy(), "logits": logits.cpu().numpy()}
    out.update({k: g[off: off + int(np.prod(shape))].reshape(shape) for k, (off, shape) in layout.items()})
    return out


def host(w, table, users, items, labels, dtype):
    loss, logits, grads = ncf_head_grad_host(w, table, users, items, labels, dtype)
    return dict(grads, loss=np.asarray([loss]), logits=logits)


@pytest.fixture(scope="module", params=HEADS, ids=lambda h: f"f{h[0]}-L{h[1]}-{h[2]}")
def head(request):
    factor, num_layers, kind = request.param
    w, table = random_head(factor, num_layers, kind, USER_NUM, ITEM_NUM, seed=2000 + 10 * factor + num_layers)
    rng = np.random.default_rng(17)
    users, items = rng.integers(0, USER_NUM - 1, size=NS[-1]), rng.integers(0, ITEM_NUM - 1, size=NS[-1])
    mixed = (rng.random(NS[-1]) < 0.4).astype(np.float32)
    fn, layout = device_grad(w, table, request.param, USER_NUM)
    return dict(shape=request.param, w=w, table=table, users=users, items=items, mixed=mixed, fn=fn, layout=layout)


def check_case(h, w, users, items, labels, what):
    got = split(*run(h["fn"], users, items, labels), h["layout"])
    o64, r32 = host(w, h["table"], users, items, labels, np.float64), host(w, h["table"], users, items, labels, np.float32)
    assert all(np.isfinite(v).all() for v in got.values()), what
    rt = ratios(got, o64, r32)
    print(f"head {h['shape']} {what}: " + ", ".join(f"{k} {v:.2f}" for k, v in rt.items()))
    emb = [k for k in got if "embeddings" in k]
    for k in emb:                                            # untouched rows: exactly +0.0
        idx = items if k.startswith("gmf_item") else users
        untouched = np.setdiff1d(np.arange(len(got[k])), idx)
        assert len(untouched) >= 1 and (got[k][untouched].view(np.uint32) == 0).all(), (what, k)
    bad = {k: v for k, v in rt.items() if not v <= C_BOUND}
    assert not bad, (h["shape"], what, bad)
    return rt


def test_loss_logits_and_every_gradient_within_the_bound(head):
    worst = {}
    for n in NS:
        for name, labels in (("mixed", head["mixed"][:n]), ("zeros", np.zeros(n, np.float32)), ("ones", np.ones(n, np.float32))):
            rt = check_case(head, head["w"], head["users"][:n], head["items"][:n], labels, f"n {n} labels {name}")
            for k, v in rt.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(f"head {head['shape']}: largest ratios " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


def test_saturated_logits(head):
    """|logit| > 100 with every label on the wrong side: log(sigmoid) would be -inf; the loss and every gradient stay finite and in bound."""
    n = 33
    users, items = head["users"][:n], head["items"][:n]
    w = dict(head["w"])
    _, z, _ = ncf_head_grad_host(w, head["table"], users, items, np.zeros(n, np.float32))
    w["predict_layer.weight"] = (w["predict_layer.weight"] * (400.0 / np.abs(z - w["predict_layer.bias"][0]).min())).astype(np.float32)
    _, z, _ = ncf_head_grad_host(w, head["table"], users, items, np.zeros(n, np.float32))
    assert np.abs(z).min() > 100
    labels = (z < 0).astype(np.float32)
    fn, layout = device_grad(w, head["table"], head["shape"], USER_NUM)
    check_case(dict(head, fn=fn, layout=layout), w, users, items, labels, "saturated")


def test_the_same_inputs_give_the_same_bits(head):
    n = 130
    a = run(head["fn"], head["users"][:n], head["items"][:n], head["mixed"][:n])
    b = run(head["fn"], head["users"][:n], head["items"][:n], head["mixed"][:n])
    fn2, _ = device_grad(head["w"], head["table"], head["shape"], USER_NUM)      # other buffers, another workspace
    c = run(fn2, head["users"][:n], head["items"][:n], head["mixed"][:n])
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    for x, y in zip(a, c):
        assert torch.equal(x, y)


def test_the_most_pairs_one_call_takes():
    from pmgt_amd.ncf_train import NCF_TRAIN_MAX_PAIRS
    shape, user_num, item_num, n = (8, 2, "NeuMF-end"), 3000, 5000, NCF_TRAIN_MAX_PAIRS
    w, table = random_head(*shape, user_num, item_num, seed=5)
    rng = np.random.default_rng(23)
    users, items = rng.integers(1, user_num, size=n), rng.integers(0, item_num - 1, size=n)
    labels = (rng.random(n) < 0.3).astype(np.float32)
    fn, layout = device_grad(w, table, shape, user_num)
    got = split(*run(fn, users, items, labels), layout)
    o64, r32 = host(w, table, users, items, labels, np.float64), host(w, table, users, items, labels, np.float32)
    assert all(np.isfinite(v).all() for v in got.values())
    assert not got["mlp_user_embeddings.weight"][0].any() and not got["gmf_item_embeddings.weight"][-1].any()
    rt = ratios(got, o64, r32)
    print("65536 pairs: " + ", ".join(f"{k} {v:.2f}" for k, v in rt.items()))
    dense = [k for k in got if k.startswith(("mlp_layers", "predict_layer"))] + ["loss"]
    bad = {k: v for k, v in rt.items() if k not in dense and not v <= C_BOUND}
    assert not bad, bad
    # the sums over all pairs: |error| <= gamma sum_p |terms|, gamma = (terms per accumulator + tree + roundings of a term) 2^-24
    for k in dense:
        terms = _abs_sum(k, w, table, users, items, labels)
        gamma = (n / 4 + 3 + 64) * 2.0 ** -24
        err = np.abs(got[k].astype(np.float64) - o64[k])
        assert (err <= gamma * terms + 1e-30).all(), (k, float((err / (gamma * terms + 1e-30)).max()))
    with pytest.raises(ValueError, match="outside"):
        fn.reserve(n + 1)


def _abs_sum(key, w, table, users, items, labels):
    """sum_p |term_p| of the sum over pairs that makes gradient `key` (or the loss), in fp64: the measure of an in-order fp32 sum's error."""
    w64 = {k: v.astype(np.float64) for k, v in w.items()}
    n, L = len(users), 2
    hs = [np.concatenate([w64["mlp_user_embeddings.weight"][users], table.astype(np.float64)[items]], axis=1)]
    for i in range(L):
        hs.append(np.maximum(hs[-1] @ w64[f"mlp_layers.{i}.linear.weight"].T + w64[f"mlp_layers.{i}.linear.bias"], 0))
    feat = np.concatenate([w64["gmf_user_embeddings.weight"][users] * w64["gmf_item_embeddings.weight"][items], hs[-1]], axis=1)
    wp = w64["predict_layer.weight"].reshape(-1)
    z = feat @ wp + w64["predict_layer.bias"][0]
    e = np.exp(-np.abs(z))
    if key == "loss":
        return np.asarray([(np.maximum(z, 0) + np.abs(z * labels) + np.log1p(e)).sum() / n])
    dl = np.abs((np.where(z >= 0, 1 / (1 + e), e / (1 + e)) - labels) / n)
    if key == "predict_layer.weight":
        return (dl @ np.abs(feat)).reshape(1, -1)
    if key == "predict_layer.bias":
        return np.asarray([dl.sum()])
    dh = (dl[:, None] * np.abs(wp)[None, :])[:, 8:]
    for i in reversed(range(L)):
        dz = dh * (hs[i + 1] > 0)
        if key == f"mlp_layers.{i}.linear.weight":
            return dz.T @ np.abs(hs[i])
        if key == f"mlp_layers.{i}.linear.bias":
            return dz.sum(axis=0)
        dh = dz @ np.abs(w64[f"mlp_layers.{i}.linear.weight"])
    raise KeyError(key)


def test_refused_before_any_launch():
    from pmgt_amd import _lib
    lib = _lib.hip()
    buf = torch.zeros(1 << 16, device="cuda")                # table, parameters and labels: zeros
    work, loss = torch.zeros(1 << 12, device="cuda"), torch.zeros(1, device="cuda")
    ids = torch.zeros(64, dtype=torch.int64, device="cuda")
    canary = torch.full((4096,), 7777.0, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = int(lib.pmgt_ncf_train_workspace_bytes(8, 2, 0, 2))
    assert need > 0

    def call(factor=8, num_layers=2, kind=0, n=2, table=buf.data_ptr(), params=buf.data_ptr(), grads=canary.data_ptr(), users=ids.data_ptr(),
             ws=work.data_ptr(), ws_bytes=need, user_num=2, item_num=2):
        h = NcfTrainC()
        h.factor_num, h.num_layers, h.kind, h.user_num, h.item_num = factor, num_layers, kind, user_num, item_num
        h.table, h.params, h.grads = table, params, grads
        return lib.pmgt_ncf_train_grad(C.byref(h), users, ids.data_ptr(), buf.data_ptr(), n, loss.data_ptr(), 0, ws, ws_bytes, st)

    bad = [dict(factor=12), dict(factor=128), dict(num_layers=0), dict(num_layers=5), dict(factor=64, num_layers=4), dict(kind=2), dict(n=0),
           dict(n=65537), dict(table=0), dict(params=0), dict(grads=0), dict(users=0), dict(ws=0), dict(ws_bytes=need - 4),
           dict(table=buf.data_ptr() + 4), dict(grads=canary.data_ptr() + 8), dict(user_num=0), dict(item_num=0)]
    assert [call(**b) for b in bad] == [-2] * len(bad)
    assert lib.pmgt_ncf_train_workspace_bytes(8, 2, 0, 0) == -2 and lib.pmgt_ncf_train_workspace_bytes(8, 2, 0, 65537) == -2
    assert lib.pmgt_ncf_train_layout(8, 5, 0, 2, 2, None) == -2
    torch.cuda.synchronize()
    assert (canary == 7777.0).all()
    assert call() == 0                                       # all-zero parameters: logits 0, loss log 2
    torch.cuda.synchronize()
    count = int(lib.pmgt_ncf_train_layout(8, 2, 0, 2, 2, None))
    assert (canary[count:] == 7777.0).all() and abs(float(loss[0]) - np.log(2.0)) < 1e-6
