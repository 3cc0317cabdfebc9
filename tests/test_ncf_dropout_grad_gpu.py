"""pmgt_ncf_train_grad_dropout on synthetic heads: the head in training mode, its masks drawn by the counter-based RNG, against
ncf_head_grad_host under the same masks restated on the host (ncf_dropout_masks), by the measure of tests/test_ncf_train_grad_gpu.py.

Per case and per quantity (loss, logits, the head's gradient tensors and, with the table trained, item_table), with
o64 = ncf_head_grad_host(..., np.float64, masks=ncf_dropout_masks(...)) and r32 = the same in np.float32:
    max|kernel - o64| <= C max(max|r32 - o64|, 2^-22 max|o64|),   C = 4.
A mask is a multiplication by 0 or by the fp32 scale 1 / (1 - p) in both, so the error classes stay those of the entries without dropout;
one wrong keep decision, a mask drawn at another (row, column), a missing 1 / (1 - p) on the way back or an undropped operand of layer 0's
weight gradient misses by orders of magnitude.  Cases: the six heads, n in {1, 31, 33, 130}, table frozen and trained, (p_emb, p_layer) in
{(0.5, 0), (0, 0.5), (0.2, 0.3)} and one with p_layer differing per layer, step counter 0 and 7; every gradient buffer pre-filled with NaN.

THE PAIRS ARE CHOSEN WELL-CONDITIONED, on the host alone.  The gradient is discontinuous where a pre-activation crosses 0: an element whose
fp64 value lies inside the fp32 rounding error of its sum passes the ReLU in one summation order and not in another, and the whole gradient
of that element -- O(1) -- is then "error" by a measure that scales with 2^-24.  64 mask sets x 33 280 pre-activations of the widest layer
meet such an element now and then (the first pair list drawn did: head (64, 3, NeuMF-end), p_emb 0.5, step 7, pair 118, feature 70 of layer
0: -3.2e-7 in fp64, -3.0e-7 in fp32 numpy, above 0 in the kernel's order; every quantity that does not pass that element stayed below 2.7).
So a pair of the list (a row of every site) is drawn again, from the same generator, until for every mask set of the test and every layer
    |a64| > 8 max|a32 - a64| on the whole row     (a = the layer's pre-activations under the masks, in fp64 and in fp32 numpy, the
                                                   maximum over the layer; 8 = 2 C)
which is a property of the reference and its own fp32 error, decided before the device computes anything.
Measured on the MI355X (one run), the largest ratio of any quantity per head: 1.06, 3.02, 1.84, 2.53, 2.69, 3.18 (per quantity: DESIGN.md row f9)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.ncf_head import TABLE_KEY, head_layout, ncf_dropout_keep, ncf_dropout_masks, ncf_head_grad_host
from pmgt_amd.ncf_train import NcfDropoutC, NcfHeadGrad, NcfTrainC
from tests.test_ncf_train_grad_gpu import C_BOUND, HEADS, ITEM_NUM, NS, USER_NUM, flatten, ratios
from tests.test_recommend_cpu import random_head

pytestmark = pytest.mark.gpu

SEED = 0x1234_5678_9ABC                                      # (above 2^32: both halves of the seed take part)
PS = [(0.5, 0.0), (0.0, 0.5), (0.2, 0.3), (0.1, [0.6, 0.0, 0.3, 0.45])]      # the last: p_layer differs per layer, one of them 0
STEPS = (0, 7)


def test_the_device_masks_of_the_ncf_sites_are_the_host_masks():
    lib = _lib.hip()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sites = [_lib.NCF_SITE_EMB, _lib.NCF_SITE_GMF] + [_lib.NCF_SITE_LAYER + i for i in range(4)]
    for seed, step in ((SEED, 0), (-3, 7)):
        rng = torch.tensor([seed, step], dtype=torch.int64, device="cuda")
        for site in sites:
            for p, rows, cols in ((0.1, 130, 512), (0.5, 33, 30), (0.8, 31, 8)):
                out = torch.full((rows, cols), 9, dtype=torch.uint8, device="cuda")
                _lib.check(lib.pmgt_op_dropout_keep(rng.data_ptr(), p, site, rows, cols, out.data_ptr(), st))
                assert np.array_equal(out.cpu().numpy().astype(bool), ncf_dropout_keep(seed, step, site, rows, cols, p)), (site, p, seed)


def make_fn(h, trained, p_emb, p_layer, rng):
    """An NcfHeadGrad over the world's parameters with buffers of its own, NaN-filled; p_layer cut to the head's layers"""
    count = h["count"]
    nan = lambda *size: torch.full(size, float("nan"), device="cuda")
    if isinstance(p_layer, list):
        p_layer = p_layer[:h["shape"][1]]
    drop = None if rng is None else (rng, p_emb, p_layer)
    return NcfHeadGrad(*h["shape"], h["user_num"], h["table_d"], h["flat"], nan(count), table_grad=nan(*h["table"].shape) if trained else None,
                       dropout=drop)


def run(fn, users, items, labels):
    fn.grads.fill_(float("nan"))                             # written whole: no NaN may survive
    if fn.table_grad is not None:
        fn.table_grad.fill_(float("nan"))
    loss, logits = fn(torch.from_numpy(users).cuda(), torch.from_numpy(items).cuda(), torch.from_numpy(labels).cuda())
    return loss.clone(), logits.clone(), fn.grads.clone(), None if fn.table_grad is None else fn.table_grad.clone()


def split(raw, layout):
    loss, logits, grads, table_grad = raw
    g = grads.cpu().numpy()
    out = {"loss": loss.cpu().numpy(), "logits": logits.cpu().numpy()}
    if table_grad is not None:
        out[TABLE_KEY] = table_grad.cpu().numpy()
    out.update({k: g[off: off + int(np.prod(shape))].reshape(shape) for k, (off, shape) in layout.items()})
    return out


def host(h, users, items, labels, dtype, trained, masks):
    loss, logits, grads = ncf_head_grad_host(h["w"], h["table"], users, items, labels, dtype, table_grad=trained, masks=masks)
    return dict(grads, loss=np.asarray([loss]), logits=logits)


def pre_activations(w, table, users, items, masks, dtype):
    """[a_0, .., a_(L-1)]: W_l h_l + b_l of the head under `masks`, before the layer's mask and the ReLU"""
    m = {k: keep.astype(dtype) * dtype(scale) for k, (keep, scale) in masks.items()}
    h = np.concatenate([w["mlp_user_embeddings.weight"][users], table[items]], axis=1).astype(dtype) * m["emb"]
    out = []
    for i in range(sum(1 for k in m if k.startswith("layer"))):
        out.append(h @ w[f"mlp_layers.{i}.linear.weight"].astype(dtype).T + w[f"mlp_layers.{i}.linear.bias"].astype(dtype))
        h = np.maximum(out[-1] * m[f"layer{i}"], 0)
    return out


def ill_conditioned_rows(shape, w, table, users, items):
    """bool [n]: the pairs with a pre-activation, under some mask set of the test, within 8 x the fp32 error of its layer from 0 (rows are
    pairs and the masks are indexed by the row: n = 130 covers every smaller n)"""
    bad = np.zeros(len(users), dtype=bool)
    for p_emb, p_layer in PS:
        pl = p_layer[:shape[1]] if isinstance(p_layer, list) else p_layer
        for step in STEPS:
            masks = ncf_dropout_masks(SEED, step, len(users), *shape, p_emb, pl)
            for a64, a32 in zip(pre_activations(w, table, users, items, masks, np.float64), pre_activations(w, table, users, items, masks, np.float32)):
                bad |= ~(np.abs(a64).min(axis=1) > 8 * np.abs(a32 - a64).max())
    return bad


@functools.lru_cache(maxsize=None)
def world(shape, user_num=USER_NUM, item_num=ITEM_NUM):
    w, table = random_head(*shape, user_num, item_num, seed=3000 + 10 * shape[0] + shape[1])
    layout, count = head_layout(*shape, user_num, item_num)
    rng = np.random.default_rng(29)
    users, items = rng.integers(0, user_num - 1, size=NS[-1]), rng.integers(0, item_num - 1, size=NS[-1])
    labels = (rng.random(NS[-1]) < 0.4).astype(np.float32)
    for _ in range(64):
        bad = np.nonzero(ill_conditioned_rows(shape, w, table, users, items))[0]
        if len(bad) == 0:
            break
        print(f"head {shape}: pairs {bad.tolist()} drawn again")
        users[bad], items[bad] = rng.integers(0, user_num - 1, size=len(bad)), rng.integers(0, item_num - 1, size=len(bad))
    else:
        raise AssertionError(f"no well-conditioned pair list for head {shape}")
    return dict(shape=shape, w=w, table=table, layout=layout, count=count, users=users, items=items, labels=labels, user_num=user_num,
                flat=torch.from_numpy(flatten(w, layout, count)).cuda(), table_d=torch.from_numpy(table).cuda())


@pytest.fixture(scope="module", params=HEADS, ids=lambda h: f"f{h[0]}-L{h[1]}-{h[2]}")
def head(request):
    return world(request.param)


def test_loss_logits_and_every_gradient_within_the_bound_under_the_host_masks(head):
    factor, num_layers, kind = head["shape"]
    rng = torch.tensor([SEED, 0], dtype=torch.int64, device="cuda")
    worst, bad = {}, {}
    for p_emb, p_layer in PS:
        pl = p_layer[:num_layers] if isinstance(p_layer, list) else p_layer
        for trained in (False, True):
            fn = make_fn(head, trained, p_emb, p_layer, rng)
            for step in STEPS:
                rng[1] = step
                for n in NS:
                    users, items, labels = head["users"][:n], head["items"][:n], head["labels"][:n]
                    got = split(run(fn, users, items, labels), head["layout"])
                    masks = ncf_dropout_masks(SEED, step, n, factor, num_layers, kind, p_emb, pl)
                    o64 = host(head, users, items, labels, np.float64, trained, masks)
                    r32 = host(head, users, items, labels, np.float32, trained, masks)
                    what = f"p {p_emb} {pl} trained {trained} step {step} n {n}"
                    assert sorted(got) == sorted(o64) and all(np.isfinite(v).all() for v in got.values()), what
                    for k in [k for k in got if "embeddings" in k or k == TABLE_KEY]:      # untouched rows: exactly +0.0
                        idx = items if k.startswith("gmf_item") or k == TABLE_KEY else users
                        untouched = np.setdiff1d(np.arange(len(got[k])), idx)
                        assert len(untouched) >= 1 and (got[k][untouched].view(np.uint32) == 0).all(), (what, k)
                    for k, v in ratios(got, o64, r32).items():
                        worst[k] = max(worst.get(k, 0.0), v)
                        if not v <= C_BOUND:
                            bad[(what, k)] = v
    print(f"head {head['shape']}: largest ratios " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    assert not bad, (head["shape"], bad)


@pytest.mark.parametrize("shape", [(8, 1, "MLP"), (16, 2, "NeuMF-end"), (64, 3, "NeuMF-end")], ids=lambda h: f"f{h[0]}-L{h[1]}-{h[2]}")
def test_dropped_columns_of_the_embedding_rows_are_exactly_zero(shape):
    """p_emb = 0.5, p_layer = 0, all users distinct and all items distinct: a pair's row of mlp_user_embeddings' gradient and of the table's
    is m_e times a dense vector, so it is == 0 on every dropped column (and the GMF rows on the dropped columns of the gmf mask)."""
    n, num = 33, 40
    h = world(shape, num, num)
    factor, num_layers, kind = shape
    d = factor << (num_layers - 1)
    perm = np.random.default_rng(5)
    users, items = perm.permutation(num - 1)[:n].astype(np.int64), perm.permutation(num - 1)[:n].astype(np.int64)      # row 39 never appears
    rng = torch.tensor([SEED, 7], dtype=torch.int64, device="cuda")
    got = split(run(make_fn(h, True, 0.5, 0.0, rng), users, items, h["labels"][:n]), h["layout"])
    masks = ncf_dropout_masks(SEED, 7, n, factor, num_layers, kind, 0.5, 0.0)
    keep = masks["emb"][0]
    for key, ids, kp in (("mlp_user_embeddings.weight", users, keep[:, :d]), (TABLE_KEY, items, keep[:, d:])) + \
            ((("gmf_user_embeddings.weight", users, masks["gmf"][0]), ("gmf_item_embeddings.weight", items, masks["gmf"][0]))
             if kind == "NeuMF-end" else ()):
        rows = got[key][ids]
        assert (rows[~kp] == 0).all() and not kp.all() and kp.any(), key
        assert (rows[kp] != 0).mean() > 0.9, key             # (a seeded dense head: the kept columns carry a gradient)
        untouched = np.setdiff1d(np.arange(num), ids)
        assert len(untouched) >= 1 and (got[key][untouched].view(np.uint32) == 0).all(), key


def test_every_p_zero_is_the_entries_without_dropout_bit_for_bit(head):
    rng = torch.tensor([SEED, 3], dtype=torch.int64, device="cuda")
    for n in (33, 130):
        args = (head["users"][:n], head["items"][:n], head["labels"][:n])
        for trained in (False, True):
            new, old = run(make_fn(head, trained, 0.0, 0.0, rng), *args), run(make_fn(head, trained, 0.0, 0.0, None), *args)
            assert all(torch.equal(a, b) for a, b in zip(new[:3], old[:3])), (head["shape"], n, trained)
            assert (new[3] is None and old[3] is None) if not trained else torch.equal(new[3], old[3])


def test_a_pure_function_of_inputs_seed_and_step(head):
    n = 130
    args = (head["users"][:n], head["items"][:n], head["labels"][:n])
    rng = torch.tensor([SEED, 7], dtype=torch.int64, device="cuda")
    fn = make_fn(head, True, 0.2, 0.3, rng)
    a, b = run(fn, *args), run(fn, *args)
    c = run(make_fn(head, True, 0.2, 0.3, rng.clone()), *args)      # other buffers, another workspace, another rng tensor
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
    rng[1] = 8
    other_step = run(fn, *args)
    rng[1], rng[0] = 7, SEED + 1
    other_seed = run(fn, *args)
    assert not torch.equal(a[1], other_step[1]) and not torch.equal(a[1], other_seed[1]) and not torch.equal(other_step[1], other_seed[1])
    rng[0] = SEED
    assert all(torch.equal(x, y) for x, y in zip(a, run(fn, *args)))


def test_refused_before_any_launch():
    lib = _lib.hip()
    buf = torch.zeros(1 << 16, device="cuda")                # table, parameters and labels: zeros
    work, loss = torch.zeros(1 << 12, device="cuda"), torch.zeros(1, device="cuda")
    ids = torch.zeros(64, dtype=torch.int64, device="cuda")
    rng = torch.tensor([5, 0, 0], dtype=torch.int64, device="cuda")
    canary, canary_t = torch.full((4096,), 7777.0, device="cuda"), torch.full((4096,), 5555.0, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    need, need_frozen = int(lib.pmgt_ncf_train_table_workspace_bytes(8, 2, 0, 2)), int(lib.pmgt_ncf_train_workspace_bytes(8, 2, 0, 2))

    def call(factor=8, num_layers=2, kind=0, n=2, table=buf.data_ptr(), params=buf.data_ptr(), grads=canary.data_ptr(), users=ids.data_ptr(),
             table_grad=canary_t.data_ptr(), ws=work.data_ptr(), ws_bytes=need, user_num=2, item_num=2, rng_ptr=rng.data_ptr(), p_emb=0.5,
             p_layer=(0.5, 0.5, 0.0, 0.0), drop=True):
        h = NcfTrainC()
        h.factor_num, h.num_layers, h.kind, h.user_num, h.item_num = factor, num_layers, kind, user_num, item_num
        h.table, h.params, h.grads = table, params, grads
        dr = NcfDropoutC(rng_ptr, p_emb)
        for i, p in enumerate(p_layer):
            dr.p_layer[i] = p
        return lib.pmgt_ncf_train_grad_dropout(C.byref(h), users, ids.data_ptr(), buf.data_ptr(), n, loss.data_ptr(), 0, table_grad,
                                               C.byref(dr) if drop else None, ws, ws_bytes, st)

    nan = float("nan")
    bad = [  # what the two entries without dropout refuse
           (dict(factor=12), "factor_num"), (dict(num_layers=5), "num_layers"), (dict(factor=64, num_layers=4), "above 256"), (dict(kind=2), "kind"),
           (dict(n=0), "n = 0"), (dict(n=65537), "n = 65537"), (dict(table=0), "NULL buffer"), (dict(grads=0), "NULL buffer"),
           (dict(users=0), "NULL buffer"), (dict(ws=0), "NULL buffer"), (dict(ws_bytes=need - 4), "workspace"),
           (dict(ws_bytes=need_frozen), "workspace"), (dict(table=buf.data_ptr() + 4), "aligned"),
           (dict(table_grad=canary_t.data_ptr() + 8), "aligned"), (dict(user_num=0), "user_num"), (dict(item_num=0), "item_num"),
           # its own
           (dict(drop=False), "NULL drop"), (dict(p_emb=1.0), "p_emb"), (dict(p_emb=-0.1), "p_emb"), (dict(p_emb=nan), "p_emb"),
           (dict(p_layer=(0.5, 1.0, 0.0, 0.0)), r"p_layer\[1\]"), (dict(p_layer=(nan, 0.5, 0.0, 0.0)), r"p_layer\[0\]"),
           (dict(p_layer=(0.0, -1.0, 0.0, 0.0)), r"p_layer\[1\]"), (dict(rng_ptr=0), "seed, step"), (dict(rng_ptr=rng.data_ptr() + 4), "seed, step"),
           (dict(rng_ptr=0, p_emb=0.0, p_layer=(0.0, 0.3, 0.0, 0.0)), "seed, step")]
    import re
    for kw, text in bad:
        assert call(**kw) == -2, kw
        assert re.search(text, lib.pmgt_last_error().decode()), (kw, lib.pmgt_last_error().decode())
    torch.cuda.synchronize()
    assert (canary == 7777.0).all() and (canary_t == 5555.0).all()
    # a p behind the head's last layer is not read; every p 0 needs no rng; a frozen table takes the smaller workspace
    assert call(p_layer=(0.5, 0.5, 7.0, nan)) == 0 and call(rng_ptr=0, p_emb=0.0, p_layer=(0.0, 0.0, 0.0, 0.0)) == 0
    assert call(table_grad=0, ws_bytes=need_frozen) == 0
    assert call() == 0                                       # all-zero parameters: logits 0, loss log 2, gradients of zeros
    torch.cuda.synchronize()
    count = int(lib.pmgt_ncf_train_layout(8, 2, 0, 2, 2, None))
    assert (canary[count:] == 7777.0).all() and abs(float(loss[0]) - np.log(2.0)) < 1e-6
    assert not canary_t[:2 * 16].any() and (canary_t[2 * 16:] == 5555.0).all()
