"""pmgt_dcn_train_grad and pmgt_dcn_forward on synthetic models: loss, logits and every gradient tensor against dcn_head_grad_host in fp64,
with the error of the same formula in fp32 numpy as the measure (tests/dcn_util.py, where the measure, the floor of the degenerate
tensors and the choice of well-conditioned pairs are stated; tests/test_dcn_measure_cpu.py checks that measure on the CPU with a second
fp32 realisation).

Per case and per quantity:  max|kernel - o64| <= 4 max(max|r32 - o64|, floor).
Cases: the six models (factor_num, deep layers, cross layers, LayerNorm) of dcn_util.HEADS -- D from 32 to 512, one to four deep layers,
one to six cross layers, widths below, at and above the 32-wide MFMA block and the 64-lane row --, n in {1, 31, 33, 130} (below, across
and above the 32-pair tile; four tiles and a remainder), labels mixed / all 0 / all 1; 5 users and 7 items with pairs drawn from 4 x 6:
duplicates are forced, user 4 and item 6 never appear and their gradient rows must be exactly +0.0.  The gradient and logit buffers are
pre-filled with NaN.

The largest case the entries take (65 536 pairs) runs once on (8, 2, 3, on) with 3 000 users and 5 000 items: the per-pair quantities (logits,
embedding rows) by the measure above, the sums over all pairs by the bound of an in-order fp32 sum, (n / 4 + 3 + 64) 2^-24 sum_p |terms|
per element (n / 4 terms per accumulator, the tree of four, 64 for the roundings inside a term), the terms' magnitudes from abs_grad.
Measured on the MI355X (one run), the largest ratio of any quantity per model: 1.58, 2.07, 1.28, 3.81, 2.96, 2.47 (per quantity: DESIGN.md
row f10); saturated 0.91 and 1.64; at 65 536 pairs logits 1.00, both tables 0.97, 45 pairs drawn again."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.dcn_head import ITEM_KEY, USER_KEY, dcn_head_grad_host, dcn_layout
from pmgt_amd.dcn_train import DcnGrad
from tests.dcn_util import (C_BOUND, EPS, HEADS, ITEM_NUM, NS, USER_NUM, abs_grad, flatten, head_id, host, label_sets, ratios, split, world)

pytestmark = pytest.mark.gpu


def device_grad(w, shape, user_num, item_num):
    layout, count = dcn_layout(*shape, user_num, item_num)
    params = torch.from_numpy(flatten(w, layout, count)).cuda()
    return DcnGrad(*shape, EPS, user_num, item_num, params, torch.full((count,), float("nan"), device="cuda")), layout


def run(fn, users, items, labels):
    fn.grads.fill_(float("nan"))                             # the buffer is written whole: no NaN may survive
    logits = torch.full((len(users),), float("nan"), device="cuda")
    loss, _ = fn(torch.from_numpy(users).cuda(), torch.from_numpy(items).cuda(), torch.from_numpy(labels).cuda(), logits=logits)
    return loss.clone(), logits, fn.grads.clone()


@pytest.fixture(scope="module", params=HEADS, ids=head_id)
def head(request):
    h = world(request.param)
    fn, layout = device_grad(h["w"], h["shape"], USER_NUM, ITEM_NUM)
    return dict(h, fn=fn)


def check_case(h, w, users, items, labels, what):
    got = split(*run(h["fn"], users, items, labels), h["layout"])
    o64, r32 = host(w, users, items, labels, np.float64), host(w, users, items, labels, np.float32)
    assert sorted(got) == sorted(o64) and all(np.isfinite(v).all() for v in got.values()), what
    rt = ratios(got, o64, r32, h["shape"], abs_grad(w, users, items, labels))
    print(f"{head_id(h['shape'])} {what}: " + ", ".join(f"{k} {v:.2f}" for k, v in rt.items()))
    for k, ids in ((USER_KEY, users), (ITEM_KEY, items)):    # untouched rows: exactly +0.0
        untouched = np.setdiff1d(np.arange(len(got[k])), ids)
        assert len(untouched) >= 1 and (got[k][untouched].view(np.uint32) == 0).all(), (what, k)
    bad = {k: v for k, v in rt.items() if not v <= C_BOUND}
    assert not bad, (h["shape"], what, bad)
    return rt


def test_loss_logits_and_every_gradient_within_the_bound(head):
    worst = {}
    for n in NS:
        assert head["redrawn"][:n].sum() * 8 <= n            # at most 1 pair in 8 was drawn again
        for name, labels in label_sets(head, n):
            rt = check_case(head, head["w"], head["users"][:n], head["items"][:n], labels, f"n {n} labels {name}")
            for k, v in rt.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(f"{head_id(head['shape'])}: largest ratios " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


def test_the_forward_entry_gives_the_gradient_entry_s_logits_bit_for_bit(head):
    for n in NS:
        users, items = torch.from_numpy(head["users"][:n]).cuda(), torch.from_numpy(head["items"][:n]).cuda()
        _, logits, _ = run(head["fn"], head["users"][:n], head["items"][:n], head["labels"][:n])
        fwd = DcnGrad(*head["shape"], EPS, USER_NUM, ITEM_NUM, head["fn"].params)      # no gradient buffer, a workspace of its own
        out = fwd.forward(users, items, logits=torch.full((n,), float("nan"), device="cuda"))
        assert torch.equal(out, logits) and torch.isfinite(out).all(), n


def test_the_same_inputs_give_the_same_bits(head):
    n = 130
    args = (head["users"][:n], head["items"][:n], head["labels"][:n])
    a, b = run(head["fn"], *args), run(head["fn"], *args)
    fn2, _ = device_grad(head["w"], head["shape"], USER_NUM, ITEM_NUM)      # other buffers, another workspace
    c = run(fn2, *args)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


@pytest.mark.parametrize("shape", [h for h in HEADS if not h[3]], ids=head_id)
def test_saturated_logits(shape):
    """|logit| > 100 with every label on the wrong side (LayerNorm off): log(sigmoid) would be -inf; the loss and every gradient stay
    finite and in bound."""
    h = world(shape)
    n = 33
    users, items = h["users"][:n], h["items"][:n]
    w = dict(h["w"])
    _, z, _ = dcn_head_grad_host(w, users, items, np.zeros(n, np.float32))
    w["output_layer.weight"] = (w["output_layer.weight"] * (400.0 / np.abs(z - w["output_layer.bias"][0]).min())).astype(np.float32)
    _, z, _ = dcn_head_grad_host(w, users, items, np.zeros(n, np.float32))
    assert np.abs(z).min() > 100
    labels = (z < 0).astype(np.float32)
    fn, layout = device_grad(w, shape, USER_NUM, ITEM_NUM)
    check_case(dict(h, fn=fn), w, users, items, labels, "saturated")


def test_the_most_pairs_one_call_takes():
    shape, user_num, item_num, n = (8, 2, 3, True), 3000, 5000, _lib.DCN_MAX_PAIRS
    h = world(shape, user_num, item_num, n, seed=23)         # (well-conditioned by the same two rules, at most 1 pair in 8 drawn again)
    w, users, items, labels = h["w"], h["users"], h["items"], h["labels"]
    print(f"65536 pairs: {int(h['redrawn'].sum())} drawn again")
    fn, layout = device_grad(w, shape, user_num, item_num)
    got = split(*run(fn, users, items, labels), layout)
    o64, r32 = host(w, users, items, labels, np.float64), host(w, users, items, labels, np.float32)
    mags = abs_grad(w, users, items, labels)
    assert all(np.isfinite(v).all() for v in got.values())
    assert not got[USER_KEY][-1].any() and not got[ITEM_KEY][-1].any()
    rt = ratios(got, o64, r32, shape, mags)
    print("65536 pairs: " + ", ".join(f"{k} {v:.2f}" for k, v in rt.items()))
    per_pair = ("logits", USER_KEY, ITEM_KEY)
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
    canary, logits = torch.full((8192,), 7777.0, device="cuda"), torch.full((64,), 5555.0, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = int(lib.pmgt_dcn_workspace_bytes(8, 2, 3, 1, 2))
    assert 0 < need <= work.numel() * 4

    def call(factor=8, deep=2, cross=3, ln=1, eps=1e-12, n=2, params=buf.data_ptr(), grads=canary.data_ptr(), users=ids.data_ptr(),
             labels=buf.data_ptr(), ws=work.data_ptr(), ws_bytes=need, user_num=2, item_num=2, out=logits.data_ptr(), lossp=loss.data_ptr(),
             forward=False):
        h = _lib.DcnHeadC(factor, deep, cross, ln, eps, 0, user_num, item_num, params, grads)
        if forward:
            return lib.pmgt_dcn_forward(C.byref(h), users, ids.data_ptr(), n, out, ws, ws_bytes, st)
        return lib.pmgt_dcn_train_grad(C.byref(h), users, ids.data_ptr(), labels, n, lossp, out, ws, ws_bytes, st)

    nan = float("nan")
    bad = [(dict(factor=12), "factor_num"), (dict(deep=0), "deep_layers"), (dict(deep=5), "deep_layers"), (dict(factor=64, deep=3), "above 256"),
           (dict(cross=0), "cross_layers"), (dict(cross=7), "cross_layers"), (dict(ln=2), "use_layer_norm"), (dict(n=0), "n = 0"),
           (dict(n=65537), "n = 65537"), (dict(params=0), "NULL buffer"), (dict(grads=0), "NULL buffer"), (dict(users=0), "NULL buffer"),
           (dict(labels=0), "NULL buffer"), (dict(lossp=0), "NULL buffer"), (dict(ws=0), "NULL buffer"), (dict(ws_bytes=need - 4), "workspace"),
           (dict(params=buf.data_ptr() + 4), "aligned"), (dict(grads=canary.data_ptr() + 8), "aligned"), (dict(ws=work.data_ptr() + 4), "aligned"),
           (dict(user_num=0), "user_num"), (dict(item_num=0), "item_num"), (dict(eps=nan), "layer_norm_eps"), (dict(eps=-1e-6), "layer_norm_eps")]
    for kw, text in bad:
        assert call(**kw) == -2, kw
        assert re.search(text, lib.pmgt_last_error().decode()), (kw, lib.pmgt_last_error().decode())
    for kw, text in ((dict(out=0), "NULL buffer"), (dict(n=65537), "n = 65537"), (dict(ws_bytes=need - 4), "workspace"), (dict(eps=nan), "layer_norm_eps"),
                     (dict(factor=64, deep=3), "above 256")):
        assert call(forward=True, **kw) == -2, kw
        assert re.search(text, lib.pmgt_last_error().decode()), (kw, lib.pmgt_last_error().decode())
    for args in ((12, 2, 3, 1, 2), (8, 2, 3, 1, 0), (8, 2, 3, 1, 65537), (8, 5, 3, 0, 2)):
        assert lib.pmgt_dcn_workspace_bytes(*args) == -2
    assert lib.pmgt_dcn_layout(8, 2, 7, 1, 2, 2, None) == -2 and lib.pmgt_dcn_layout(8, 2, 3, 1, 0, 2, None) == -2
    torch.cuda.synchronize()
    assert (canary == 7777.0).all() and (logits == 5555.0).all() and float(loss[0]) == 3333.0
    # a NULL logits is allowed by the gradient entry, a NULL grads by the forward entry; eps = 0 is a value like any other
    assert call(out=0) == 0 and call(forward=True, grads=0) == 0 and call(eps=0.0, ln=0) == 0
    assert call() == 0                                       # all-zero parameters: logits 0, loss log 2
    torch.cuda.synchronize()
    count = int(lib.pmgt_dcn_layout(8, 2, 3, 1, 2, 2, None))
    assert (canary[count:] == 7777.0).all() and abs(float(loss[0]) - np.log(2.0)) < 1e-6
    assert not logits[:2].any() and (logits[2:] == 5555.0).all()
