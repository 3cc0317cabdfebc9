"""pmgt_ncf_model_train_grad on synthetic models: loss, logits and every gradient tensor against ncf_model_grad_host in fp64, with the error
of the same formula in fp32 numpy as the measure (tests/dcn_util.py's ratios and C_BOUND; tests/ncf_model_util.py states the choice of
well-conditioned pairs, and tests/test_ncf_model_measure_cpu.py checks the measure on the CPU with a second fp32 realisation).

Per case and per quantity:  max|kernel - o64| <= 4 max(max|r32 - o64|, 2^-22 max|o64|).
Cases: the seven models (factor_num, num_layers, kind, LayerNorm) of ncf_model_util.HEADS -- d from 8 (below the 32-wide MFMA block) to
256 (the widest; four floats a lane of the row work), one to four layers, MLP and NeuMF-end with LayerNorm, and kind GMF --, n in
{1, 31, 33, 130} (below, across and above the 32-pair tile; four tiles and a remainder), labels mixed / all 0 / all 1, the items trained
and frozen; 5 users and 7 items with pairs drawn from 4 x 6: duplicates are forced, user 4 and item 6 never appear and their gradient
rows must be exactly +0.0.  The gradient and logit buffers are pre-filled with NaN.

The largest case the entry takes (65 536 pairs) runs once on (8, 2, NeuMF-end, on) with 3 000 users and 5 000 items, judged as
tests/test_dcn_grad_gpu.py judges the DCN: the per-pair quantities (logits, embedding rows) by the measure above, the sums over all pairs
by the bound of an in-order fp32 sum, (n / 4 + 3 + 64) 2^-24 sum_p |terms| per element.
Measured on the MI355X (one run), the largest ratio of any quantity per model, in HEADS' order: 1.41, 1.57, 1.66, 2.07, 1.53, 1.12, 1.00; with
dropout, in DROP_HEADS' order: 2.97, 2.99, 1.96, 0.99; at 65 536 pairs logits 0.66, the four tables 1.01 at most, 10 pairs drawn again.  (With
ONE chain of MFMA steps per product the same lists gave 2.34, 1.52, 2.07, 3.23, 3.73 and single misses of 4.1 to 5.7: ops/ncf_model_train.hip
says why it has four.)"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.ncf_model import ITEM_GMF, ITEM_MLP, USER_GMF, USER_MLP, ncf_model_layout
from pmgt_amd.ncf_model_train import NcfModelGrad
from pmgt_amd.ncf_train import NcfHeadGrad
from tests.dcn_util import C_BOUND, ratios
from tests.ncf_model_util import (DROP_HEADS, DROP_STEPS, DROPS, EPS, HEADS, ITEM_NUM, NS, SEED, USER_NUM, abs_grad, cut, drop_world, flatten, head_id,
                                  host, label_sets, masks_of, split, world)

pytestmark = pytest.mark.gpu
TABLES = (USER_MLP, ITEM_MLP, USER_GMF, ITEM_GMF)


def device_grad(w, shape, user_num, item_num, train_items=True, dropout=None):
    layout, count = ncf_model_layout(*shape, user_num, item_num, train_items)
    params = torch.from_numpy(flatten(w, layout, count)).cuda()
    table = None if train_items or shape[2] == "GMF" else torch.from_numpy(w[ITEM_MLP]).cuda()
    fn = NcfModelGrad(*shape, EPS, user_num, item_num, params, torch.full((count,), float("nan"), device="cuda"), train_items=train_items,
                      item_table=table, dropout=dropout)
    return fn, layout


def run(fn, users, items, labels):
    fn.grads.fill_(float("nan"))                             # the named tensors are written whole: no NaN may survive in them
    logits = torch.full((len(users),), float("nan"), device="cuda")
    loss, _ = fn(torch.from_numpy(users).cuda(), torch.from_numpy(items).cuda(), torch.from_numpy(labels).cuda(), logits=logits)
    return loss.clone(), logits, fn.grads.clone()


@pytest.fixture(scope="module", params=HEADS, ids=head_id)
def head(request):
    h = world(request.param)
    fn, layout = device_grad(h["w"], h["shape"], USER_NUM, ITEM_NUM)
    frozen, frozen_layout = device_grad(h["w"], h["shape"], USER_NUM, ITEM_NUM, train_items=False)
    return dict(h, fn=fn, layout=layout, frozen=frozen, frozen_layout=frozen_layout)


def check_case(h, fn, layout, train_items, users, items, labels, what, masks=None):
    w, kind = h["w"], h["kind"]
    got = split(*run(fn, users, items, labels), layout)
    o64, r32 = (host(w, kind, users, items, labels, dt, train_items, masks) for dt in (np.float64, np.float32))
    assert sorted(got) == sorted(o64) and all(np.isfinite(v).all() for v in got.values()), what
    rt = ratios(got, o64, r32)
    print(f"{head_id(h['shape'])} {what}: " + ", ".join(f"{k} {v:.2f}" for k, v in rt.items()))
    for k in TABLES:                                         # untouched rows: exactly +0.0
        if k in got:
            untouched = np.setdiff1d(np.arange(len(got[k])), users if "user" in k else items)
            assert len(untouched) >= 1 and (got[k][untouched].view(np.uint32) == 0).all(), (what, k)
    bad = {k: v for k, v in rt.items() if not v <= C_BOUND}
    assert not bad, (h["shape"], what, bad)
    return rt


def test_loss_logits_and_every_gradient_within_the_bound(head):
    worst = {}
    for n in NS:
        assert head["redrawn"][:n].sum() * 8 <= n            # at most 1 pair in 8 was drawn again
        for name, labels in label_sets(head, n):
            for train_items in (True, False):
                fn, layout = (head["fn"], head["layout"]) if train_items else (head["frozen"], head["frozen_layout"])
                rt = check_case(head, fn, layout, train_items, head["users"][:n], head["items"][:n], labels,
                                f"n {n} labels {name} items {'trained' if train_items else 'frozen'}")
                for k, v in rt.items():
                    worst[k] = max(worst.get(k, 0.0), v)
    print(f"{head_id(head['shape'])}: largest ratios " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))
    print(f"{head_id(head['shape'])}: LARGEST {max(worst.values()):.2f}")


def test_frozen_items_give_the_bits_of_trained_items(head):
    n = 130
    args = (head["users"][:n], head["items"][:n], head["labels"][:n])
    a, b = split(*run(head["fn"], *args), head["layout"]), split(*run(head["frozen"], *args), head["frozen_layout"])
    assert sorted(b) == sorted(k for k in a if k != ITEM_MLP or head["kind"] == "GMF")
    for k in b:
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), k


def test_the_same_inputs_give_the_same_bits(head):
    n = 130
    args = (head["users"][:n], head["items"][:n], head["labels"][:n])
    a, b = run(head["fn"], *args), run(head["fn"], *args)
    fn2, _ = device_grad(head["w"], head["shape"], USER_NUM, ITEM_NUM)      # other buffers, another workspace
    fn2.reserve(4 * n)                                       # (a larger one: the offsets inside it differ from the first call's)
    c = run(fn2, *args)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)) and torch.equal(x.view(torch.int32), z.view(torch.int32))


@pytest.mark.parametrize("train_items", (True, False), ids=("trained", "frozen"))
@pytest.mark.parametrize("shape", [(16, 3, "NeuMF-end", False), (8, 2, "MLP", False), (8, 2, "NeuMF-pre", False)], ids=head_id)
@pytest.mark.parametrize("drop", (None, (0.2, [0.1, 0.3, 0.5])), ids=("nodrop", "drop"))
def test_without_layernorm_the_bits_are_the_pmgt_ncf_heads(shape, train_items, drop):
    """A model without LayerNorm of kind MLP / NeuMF-end (NeuMF-pre trains as NeuMF-end) gives the bits of NcfHeadGrad on the mapped buffers."""
    factor, layers, kind, _ = shape
    h = world(shape)
    n = 130
    layout, count = ncf_model_layout(*shape, USER_NUM, ITEM_NUM, train_items)
    head_count = layout["predict_layer.bias"][0] + 1
    rng = torch.tensor([SEED, 5], dtype=torch.int64, device="cuda")
    dropout = None if drop is None else (rng, drop[0], drop[1][:layers])
    fn, _ = device_grad(h["w"], shape, USER_NUM, ITEM_NUM, train_items, dropout)
    theirs_params, theirs_grads = fn.params.clone(), torch.full((count,), float("nan"), device="cuda")
    if train_items:
        off, size = layout[ITEM_MLP][0], ITEM_NUM * (factor << (layers - 1))
        table = theirs_params[off: off + size].view(ITEM_NUM, -1)
        table_grad = theirs_grads[off: off + size].view(ITEM_NUM, -1)
    else:
        table, table_grad = torch.from_numpy(h["w"][ITEM_MLP]).cuda(), None
    theirs = NcfHeadGrad(factor, layers, "MLP" if kind == "MLP" else "NeuMF-end", USER_NUM, table, theirs_params[:head_count],
                         theirs_grads[:head_count], table_grad=table_grad, dropout=dropout)
    args = [torch.from_numpy(a[:n]).cuda() for a in (h["users"], h["items"], h["labels"])]
    fn.grads.fill_(float("nan"))
    loss_a, logits_a = fn(*args)
    loss_b, logits_b = theirs(*args)
    assert torch.equal(loss_a, loss_b) and torch.equal(logits_a, logits_b) and torch.isfinite(logits_a).all()
    for k, (off, shp) in layout.items():
        a, b = fn.grads[off: off + int(np.prod(shp))], theirs_grads[off: off + int(np.prod(shp))]
        assert torch.isfinite(a).all() and torch.equal(a.view(torch.int32), b.view(torch.int32)), k


@pytest.mark.parametrize("shape", DROP_HEADS, ids=head_id)
def test_dropout_against_the_masked_yardstick(shape):
    h = drop_world(shape)
    layers = shape[1]
    worst = 0.0
    for p_emb, p in DROPS:
        p_layer = p if np.isscalar(p) else list(p[:layers])
        for step in DROP_STEPS:
            rng = torch.tensor([SEED, step], dtype=torch.int64, device="cuda")
            fn, layout = device_grad(h["w"], shape, USER_NUM, ITEM_NUM, True, (rng, p_emb, p_layer))
            full = masks_of(shape, NS[-1], p_emb, p_layer, step)
            for n in NS:
                assert h["redrawn"][:n].sum() * 8 <= n
                rt = check_case(h, fn, layout, True, h["users"][:n], h["items"][:n], h["labels"][:n], f"p {p_emb} / {p_layer} step {step} n {n}",
                                masks=cut(full, n))
                worst = max(worst, max(rt.values()))
    print(f"{head_id(shape)}: dropout LARGEST {worst:.2f}")


def test_with_every_p_zero_the_dropout_setting_changes_no_bit(head):
    n = 33
    args = (head["users"][:n], head["items"][:n], head["labels"][:n])
    fn, _ = device_grad(head["w"], head["shape"], USER_NUM, ITEM_NUM, True, (torch.zeros(2, dtype=torch.int64, device="cuda"), 0.0, 0.0))
    for x, y in zip(run(head["fn"], *args), run(fn, *args)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))


def test_the_most_pairs_one_call_takes():
    shape, user_num, item_num, n = (8, 2, "NeuMF-end", True), 3000, 5000, _lib.NCF_TRAIN_MAX_PAIRS
    h = world(shape, user_num, item_num, n, seed=23)         # (well-conditioned by the same rule, at most 1 pair in 8 drawn again)
    w, kind, users, items, labels = h["w"], h["kind"], h["users"], h["items"], h["labels"]
    print(f"65536 pairs: {int(h['redrawn'].sum())} drawn again")
    fn, layout = device_grad(w, shape, user_num, item_num)
    got = split(*run(fn, users, items, labels), layout)
    o64, r32 = host(w, kind, users, items, labels, np.float64), host(w, kind, users, items, labels, np.float32)
    mags = abs_grad(w, kind, users, items, labels)
    assert all(np.isfinite(v).all() for v in got.values())
    assert all(not got[k][-1].any() for k in TABLES)
    rt = ratios(got, o64, r32)
    print("65536 pairs: " + ", ".join(f"{k} {v:.2f}" for k, v in rt.items()))
    per_pair = ("logits",) + TABLES
    bad = {k: v for k, v in rt.items() if k in per_pair and not v <= C_BOUND}
    assert not bad, bad
    gamma = (n / 4 + 3 + 64) * 2.0 ** -24
    for k in got:
        if k not in per_pair:                                # the sums over all pairs: |error| <= gamma sum_p |terms|
            err = np.abs(got[k].astype(np.float64) - o64[k].reshape(got[k].shape))
            bound = gamma * mags[k].reshape(got[k].shape) + 1e-30
            assert (err <= bound).all(), (k, float((err / bound).max()))
    with pytest.raises(ValueError, match="outside"):
        fn.reserve(n + 1)


def test_refused_before_any_launch():
    lib = _lib.hip()
    buf = torch.zeros(1 << 16, device="cuda")                # parameters and labels: zeros
    work, loss = torch.zeros(1 << 14, device="cuda"), torch.full((1,), 3333.0, device="cuda")
    ids = torch.zeros(64, dtype=torch.int64, device="cuda")
    rng = torch.zeros(4, dtype=torch.int64, device="cuda")
    canary, logits = torch.full((8192,), 7777.0, device="cuda"), torch.full((64,), 5555.0, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    MLP, NEUMF, GMF, PRE = range(4)
    need = int(lib.pmgt_ncf_model_workspace_bytes(8, 2, NEUMF, 1, 1, 2))
    assert 0 < need <= work.numel() * 4

    def call(factor=8, layers=2, kind=NEUMF, ln=1, eps=1e-12, train_items=1, n=2, params=buf.data_ptr(), grads=canary.data_ptr(),
             table=buf.data_ptr(), table_grad=canary.data_ptr() + 4096 * 4, users=ids.data_ptr(), items=ids.data_ptr(), labels=buf.data_ptr(),
             ws=work.data_ptr(), ws_bytes=need, user_num=2, item_num=2, out=logits.data_ptr(), lossp=loss.data_ptr(), drop=None):
        m = _lib.NcfModelC(factor, layers, kind, ln, eps, train_items, user_num, item_num, table, params, grads, table_grad)
        d = None
        if drop is not None:
            d = _lib.NcfDropoutC(drop[0], drop[1])
            for i, p in enumerate(drop[2]):
                d.p_layer[i] = p
            d = C.byref(d)
        return lib.pmgt_ncf_model_train_grad(C.byref(m), users, items, labels, n, lossp, out, d, ws, ws_bytes, st)

    nan, r = float("nan"), rng.data_ptr()
    bad = [(dict(factor=12), "factor_num"), (dict(layers=0), "num_layers"), (dict(layers=5), "num_layers"), (dict(factor=64, layers=4), "above 256"),
           (dict(kind=4), "model kind"), (dict(kind=-1), "model kind"), (dict(eps=nan), "layer_norm_eps"), (dict(eps=-1e-6), "layer_norm_eps"),
           (dict(eps=float("inf")), "layer_norm_eps"), (dict(n=0), "n = 0"), (dict(n=65537), "n = 65537"), (dict(params=0), "NULL buffer"),
           (dict(grads=0), "NULL buffer"), (dict(table=0), "NULL buffer"), (dict(users=0), "NULL buffer"), (dict(items=0), "NULL buffer"),
           (dict(labels=0), "NULL buffer"), (dict(lossp=0), "NULL buffer"), (dict(ws=0), "NULL buffer"), (dict(table_grad=0), "NULL table_grad"),
           (dict(ws_bytes=need - 4), "workspace"), (dict(params=buf.data_ptr() + 4), "aligned"), (dict(grads=canary.data_ptr() + 8), "aligned"),
           (dict(table=buf.data_ptr() + 8), "aligned"), (dict(table_grad=canary.data_ptr() + 4), "aligned"), (dict(ws=work.data_ptr() + 4), "aligned"),
           (dict(users=ids.data_ptr() + 4), "misaligned"), (dict(labels=buf.data_ptr() + 2), "misaligned"), (dict(user_num=0), "user_num"),
           (dict(item_num=0), "item_num"), (dict(drop=(r, 1.0, [0, 0])), "p_emb"), (dict(drop=(r, nan, [0, 0])), "p_emb"),
           (dict(drop=(r, 0.0, [0, -0.1])), r"p_layer\[1\]"), (dict(drop=(0, 0.2, [0, 0])), "seed, step"),
           (dict(drop=(r + 4, 0.0, [0.5, 0])), "seed, step"), (dict(kind=GMF, drop=(0, 0.2, [0, 0])), "seed, step"),
           # the same refusals on the cases the entry hands to the PMGT_NCF head's kernels (LayerNorm off) and on kind GMF
           (dict(ln=0, n=65537), "n = 65537"), (dict(ln=0, table_grad=0), "NULL table_grad"), (dict(ln=0, ws_bytes=64), "workspace"),
           (dict(ln=0, kind=PRE, drop=(0, 0.2, [0, 0])), "seed, step"), (dict(kind=GMF, params=0), "NULL buffer"),
           (dict(kind=GMF, ws_bytes=16), "workspace")]
    for kw, text in bad:
        assert call(**kw) == -2, kw
        assert re.search(text, lib.pmgt_last_error().decode()), (kw, lib.pmgt_last_error().decode())
    for args in ((12, 2, MLP, 1, 1, 2), (8, 2, MLP, 1, 1, 0), (8, 2, MLP, 1, 1, 65537), (8, 5, GMF, 0, 0, 2), (64, 4, PRE, 1, 1, 2), (8, 2, 7, 1, 1, 2)):
        assert lib.pmgt_ncf_model_workspace_bytes(*args) == -2
    assert lib.pmgt_ncf_model_layout(8, 2, 9, 1, 1, 2, 2, None) == -2 and lib.pmgt_ncf_model_layout(8, 2, MLP, 1, 1, 0, 2, None) == -2
    assert lib.pmgt_ncf_model_workspace_bytes(64, 4, GMF, 0, 0, 2) > 0       # kind GMF: d is not limited
    torch.cuda.synchronize()
    assert (canary == 7777.0).all() and (logits == 5555.0).all() and float(loss[0]) == 3333.0
    # allowed: a NULL logits; eps = 0; kind GMF with no item table and no table_grad; every p 0 with a NULL rng; frozen items with no table_grad
    assert call(out=0) == 0 and call(eps=0.0) == 0 and call(kind=GMF, table=0, table_grad=0) == 0
    assert call(drop=(0, 0.0, [0.0, 0.0])) == 0 and call(train_items=0, table_grad=0) == 0
    assert call() == 0                                       # all-zero parameters: logits 0, loss log 2
    torch.cuda.synchronize()
    count = int(lib.pmgt_ncf_model_layout(8, 2, NEUMF, 1, 0, 2, 2, None))
    assert (canary[count: 4096] == 7777.0).all() and (canary[4096 + 2 * 16:] == 7777.0).all() and abs(float(loss[0]) - np.log(2.0)) < 1e-6
    assert not logits[:2].any() and (logits[2:] == 5555.0).all()
