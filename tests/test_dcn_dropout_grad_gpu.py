"""pmgt_dcn_train_grad_dropout on synthetic models: the DCN in training mode, its masks drawn by the counter-based RNG inside the two
launches, against dcn_head_grad_host under the same masks restated on the host (dcn_dropout_masks), by the measure of
tests/dcn_dropout_util.py (tests/dcn_util.py's, C = 4; its header states the floors of the degenerate and the nearly degenerate tensors
and the choice of well-conditioned pairs; tests/test_dcn_dropout_cpu.py checks all of it on the CPU with a second fp32 realisation).

Per case and per quantity (loss, logits, every gradient tensor), o64 / r32 = dcn_head_grad_host(masks=...) in fp64 / fp32:
    max|kernel - o64| <= 4 max(max|r32 - o64|, floor).
A mask is a multiplication by 0 or by the fp32 scale 1 / (1 - p) in both, so one wrong keep decision, a mask drawn at another (row,
column), a dropout on the wrong side of a LayerNorm, a cross mask on the added x0, a missing 1 / (1 - p) on the way back or an undropped
operand of a weight gradient misses by orders of magnitude.  Cases: the six models of dcn_util.HEADS, n in {1, 31, 33, 130}, (p_emb,
p_deep, p_cross) in {(0.2, 0, 0), (0, 0.5, 0), (0, 0, 0.5), (0.1, 0.3, 0.3)}, step counter 0 and 7, mixed labels; 5 users and 7 items with
pairs from 4 x 6 (duplicates forced; user 4 and item 6 never appear: their gradient rows are exactly +0.0); every buffer pre-filled with
NaN.  Also: the device's keep decisions at every DCN site == the host's; with p_emb = 0.5 and distinct ids the embedding-gradient rows
are == 0 on every dropped column; with every p = 0 the outputs are pmgt_dcn_train_grad's bit for bit; the call is a pure function of
(inputs, seed, step); the refusals.

MEASURED on the MI355X (one run): every case of every model is within the bound; the largest ratio of any quantity per model 1.82,
2.00, 3.01, 2.19, 2.17, 2.19 (nearly degenerate tensors with their floor: at most 1.57); per quantity: DESIGN.md row f11.
(With the in-order fp32 row sums and MFMA chains of the entries without dropout, the first form of the DROP instantiations, the cases at
n = 31, 33 and 130 passed and seven (case, quantity) at n = 1 did not: 4.07 to 5.84 on five gradient tensors, 9.29 on the one logit of
(64, 1, 6, off) -- with one pair numpy's error is that of single BLAS dot products, at the floor of the measure.  The DROP instantiations
now reduce rows in fp64 and sum MFMA chains blockwise; the bound, the references and the cases are as they were.)"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.dcn_head import ITEM_KEY, USER_KEY, dcn_layout
from pmgt_amd.dcn_train import DcnGrad
from pmgt_amd.ncf_head import ncf_dropout_keep
from tests.dcn_dropout_util import NS, PS, SEED, STEPS, abs_grad_masked, cut, host_masked, masks_of, near_keys_p, ratios_p, world
from tests.dcn_util import C_BOUND, EPS, HEADS, ITEM_NUM, USER_NUM, flatten, head_id, random_dcn, split

pytestmark = pytest.mark.gpu


def test_the_device_masks_of_the_dcn_sites_are_the_host_masks():
    lib = _lib.hip()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    sites = ([_lib.DCN_SITE_EMB] + [_lib.DCN_SITE_DEEP + l for l in range(_lib.DCN_MAX_DEEP)]
             + [_lib.DCN_SITE_CROSS + c for c in range(_lib.DCN_MAX_CROSS)])
    for seed, step in ((SEED, 0), (-3, 7)):
        rng = torch.tensor([seed, step], dtype=torch.int64, device="cuda")
        for site in sites:
            for p, rows, cols in ((0.1, 130, 512), (0.5, 33, 32), (0.8, 31, 8)):
                out = torch.full((rows, cols), 9, dtype=torch.uint8, device="cuda")
                _lib.check(lib.pmgt_op_dropout_keep(rng.data_ptr(), p, site, rows, cols, out.data_ptr(), st))
                assert np.array_equal(out.cpu().numpy().astype(bool), ncf_dropout_keep(seed, step, site, rows, cols, p)), (site, p, seed)


def make_fn(h, p, rng, user_num=USER_NUM, item_num=ITEM_NUM):
    """A DcnGrad over the world's parameters with a NaN-filled gradient buffer of its own; p = (p_emb, p_deep, p_cross) or None"""
    layout, count = dcn_layout(*h["shape"], user_num, item_num)
    params = torch.from_numpy(flatten(h["w"], layout, count)).cuda()
    return DcnGrad(*h["shape"], EPS, user_num, item_num, params, torch.full((count,), float("nan"), device="cuda"),
                   dropout=None if p is None else (rng, *p))


def run(fn, users, items, labels):
    fn.grads.fill_(float("nan"))                             # the buffer is written whole: no NaN may survive
    logits = torch.full((len(users),), float("nan"), device="cuda")
    loss, _ = fn(torch.from_numpy(users).cuda(), torch.from_numpy(items).cuda(), torch.from_numpy(labels).cuda(),
                 loss=torch.full((1,), float("nan"), device="cuda"), logits=logits)
    return loss.clone(), logits, fn.grads.clone()


@pytest.fixture(scope="module", params=HEADS, ids=head_id)
def head(request):
    return world(request.param)


def test_loss_logits_and_every_gradient_within_the_bound_under_the_host_masks(head):
    shape = head["shape"]
    rng = torch.tensor([SEED, 0], dtype=torch.int64, device="cuda")
    worst, worst_near, bad = {}, 0.0, {}
    for n in NS:
        assert head["redrawn"][:n].sum() * 8 <= n            # at most 1 pair in 8 was drawn again
    for p in PS:
        fn = make_fn(head, p, rng)
        for step in STEPS:
            rng[1] = step
            full = masks_of(shape, NS[-1], p, step)
            for n in NS:
                users, items, labels, masks = head["users"][:n], head["items"][:n], head["labels"][:n], cut(full, n)
                got = split(*run(fn, users, items, labels), head["layout"])
                o64, r32 = (host_masked(head["w"], users, items, labels, dt, masks) for dt in (np.float64, np.float32))
                what = f"p {p} step {step} n {n}"
                assert sorted(got) == sorted(o64) and all(np.isfinite(v).all() for v in got.values()), what
                for k, ids in ((USER_KEY, users), (ITEM_KEY, items)):    # untouched rows: exactly +0.0
                    untouched = np.setdiff1d(np.arange(len(got[k])), ids)
                    assert len(untouched) >= 1 and (got[k][untouched].view(np.uint32) == 0).all(), (what, k)
                for k, v in ratios_p(got, o64, r32, shape, p[2], abs_grad_masked(head["w"], users, items, labels, masks)).items():
                    worst[k] = max(worst.get(k, 0.0), v)
                    if k in near_keys_p(shape, p[2]):
                        worst_near = max(worst_near, v)
                    if not v <= C_BOUND:
                        bad[(what, k)] = v
    print(f"{head_id(shape)}: largest ratios " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()) + f"; nearly degenerate {worst_near:.2f}")
    assert not bad, (shape, bad)


@pytest.mark.parametrize("shape", [(8, 1, 1, False), (16, 1, 4, True), (16, 4, 2, True)], ids=head_id)
def test_dropped_columns_of_the_embedding_rows_are_exactly_zero(shape):
    """p_emb = 0.5, every other p 0, all users distinct and all items distinct: a pair's row of either table's gradient is m_e times a
    dense vector, so it is == 0 on every dropped column; rows no pair touches are +0.0."""
    n, num = 33, 40
    h = dict(shape=shape, w=random_dcn(*shape, num, num, seed=77), layout=dcn_layout(*shape, num, num)[0],
             labels=(np.random.default_rng(6).random(n) < 0.4).astype(np.float32))
    E = shape[0] << shape[1]
    perm = np.random.default_rng(5)
    users, items = perm.permutation(num - 1)[:n].astype(np.int64), perm.permutation(num - 1)[:n].astype(np.int64)      # row 39 never appears
    rng = torch.tensor([SEED, 7], dtype=torch.int64, device="cuda")
    p = (0.5, 0.0, 0.0)
    got = split(*run(make_fn(h, p, rng, num, num), users, items, h["labels"][:n]), h["layout"])
    keep = masks_of(shape, n, p, 7)["emb"][0]
    for key, ids, kp in ((USER_KEY, users, keep[:, :E]), (ITEM_KEY, items, keep[:, E:])):
        rows = got[key][ids]
        assert (rows[~kp] == 0).all() and not kp.all() and kp.any(), key
        assert (rows[kp] != 0).mean() > 0.9, key             # (a seeded dense model: the kept columns carry a gradient)
        untouched = np.setdiff1d(np.arange(num), ids)
        assert len(untouched) >= 1 and (got[key][untouched].view(np.uint32) == 0).all(), key


def test_every_p_zero_is_the_entry_without_dropout_bit_for_bit(head):
    rng = torch.tensor([SEED, 3], dtype=torch.int64, device="cuda")
    for n in (33, 130):
        args = (head["users"][:n], head["items"][:n], head["labels"][:n])
        new, old = run(make_fn(head, (0.0, 0.0, 0.0), rng), *args), run(make_fn(head, None, None), *args)
        assert all(torch.equal(a, b) for a, b in zip(new, old)) and torch.isfinite(new[2]).all(), (head["shape"], n)


def test_a_pure_function_of_inputs_seed_and_step(head):
    n = 130
    args = (head["users"][:n], head["items"][:n], head["labels"][:n])
    rng = torch.tensor([SEED, 7], dtype=torch.int64, device="cuda")
    p = (0.1, 0.3, 0.3)
    fn = make_fn(head, p, rng)
    a, b = run(fn, *args), run(fn, *args)
    c = run(make_fn(head, p, rng.clone()), *args)            # other buffers, another workspace, another rng tensor
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
    buf = torch.zeros(1 << 16, device="cuda")                # parameters and labels: zeros
    work, loss = torch.zeros(1 << 14, device="cuda"), torch.full((1,), 3333.0, device="cuda")
    ids = torch.zeros(64, dtype=torch.int64, device="cuda")
    rng = torch.tensor([5, 0, 0], dtype=torch.int64, device="cuda")
    canary, logits = torch.full((8192,), 7777.0, device="cuda"), torch.full((64,), 5555.0, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = int(lib.pmgt_dcn_workspace_bytes(8, 2, 3, 1, 2))
    assert 0 < need <= work.numel() * 4

    def call(factor=8, deep=2, cross=3, ln=1, eps=1e-12, n=2, params=buf.data_ptr(), grads=canary.data_ptr(), users=ids.data_ptr(),
             labels=buf.data_ptr(), ws=work.data_ptr(), ws_bytes=need, user_num=2, item_num=2, out=logits.data_ptr(), lossp=loss.data_ptr(),
             rng_ptr=rng.data_ptr(), p_emb=0.5, p_deep=(0.5, 0.5, 0.0, 0.0), p_cross=(0.5, 0.5, 0.5, 0.0, 0.0, 0.0), drop=True):
        h = _lib.DcnHeadC(factor, deep, cross, ln, eps, 0, user_num, item_num, params, grads)
        dr = _lib.DcnDropoutC(rng_ptr, p_emb)
        for i, p in enumerate(p_deep):
            dr.p_deep[i] = p
        for i, p in enumerate(p_cross):
            dr.p_cross[i] = p
        return lib.pmgt_dcn_train_grad_dropout(C.byref(h), users, ids.data_ptr(), labels, n, lossp, out, C.byref(dr) if drop else None, ws,
                                               ws_bytes, st)

    nan = float("nan")
    bad = [  # what pmgt_dcn_train_grad refuses
           (dict(factor=12), "factor_num"), (dict(deep=0), "deep_layers"), (dict(deep=5), "deep_layers"), (dict(factor=64, deep=3), "above 256"),
           (dict(cross=0), "cross_layers"), (dict(cross=7), "cross_layers"), (dict(ln=2), "use_layer_norm"), (dict(n=0), "n = 0"),
           (dict(n=65537), "n = 65537"), (dict(params=0), "NULL buffer"), (dict(grads=0), "NULL buffer"), (dict(users=0), "NULL buffer"),
           (dict(labels=0), "NULL buffer"), (dict(lossp=0), "NULL buffer"), (dict(ws=0), "NULL buffer"), (dict(ws_bytes=need - 4), "workspace"),
           (dict(params=buf.data_ptr() + 4), "aligned"), (dict(grads=canary.data_ptr() + 8), "aligned"), (dict(ws=work.data_ptr() + 4), "aligned"),
           (dict(user_num=0), "user_num"), (dict(item_num=0), "item_num"), (dict(eps=nan), "layer_norm_eps"), (dict(eps=-1e-6), "layer_norm_eps"),
           # its own
           (dict(drop=False), "NULL drop"), (dict(p_emb=1.0), "p_emb"), (dict(p_emb=-0.1), "p_emb"), (dict(p_emb=nan), "p_emb"),
           (dict(p_deep=(0.5, 1.0, 0.0, 0.0)), r"p_deep\[1\]"), (dict(p_deep=(nan, 0.5, 0.0, 0.0)), r"p_deep\[0\]"),
           (dict(p_deep=(0.0, -1.0, 0.0, 0.0)), r"p_deep\[1\]"), (dict(p_cross=(0.5, 0.5, 1.5, 0.0, 0.0, 0.0)), r"p_cross\[2\]"),
           (dict(p_cross=(nan, 0.5, 0.5, 0.0, 0.0, 0.0)), r"p_cross\[0\]"), (dict(rng_ptr=0), "seed, step"),
           (dict(rng_ptr=rng.data_ptr() + 4), "seed, step"),
           (dict(rng_ptr=0, p_emb=0.0, p_deep=(0.0, 0.0, 0.0, 0.0), p_cross=(0.0, 0.3, 0.0, 0.0, 0.0, 0.0)), "seed, step"),
           (dict(rng_ptr=0, p_emb=0.0, p_deep=(0.0, 0.3, 0.0, 0.0), p_cross=(0.0,) * 6), "seed, step")]
    for kw, text in bad:
        assert call(**kw) == -2, kw
        assert re.search(text, lib.pmgt_last_error().decode()), (kw, lib.pmgt_last_error().decode())
    torch.cuda.synchronize()
    assert (canary == 7777.0).all() and (logits == 5555.0).all() and float(loss[0]) == 3333.0
    # a p behind the model's last layer is not read; every p 0 needs no rng; a NULL logits is allowed
    assert call(p_deep=(0.5, 0.5, 7.0, nan), p_cross=(0.5, 0.5, 0.5, nan, -1.0, 2.0)) == 0
    assert call(rng_ptr=0, p_emb=0.0, p_deep=(0.0,) * 4, p_cross=(0.0,) * 6) == 0 and call(out=0) == 0
    assert call() == 0                                       # all-zero parameters: logits 0, loss log 2
    torch.cuda.synchronize()
    count = int(lib.pmgt_dcn_layout(8, 2, 3, 1, 2, 2, None))
    assert (canary[count:] == 7777.0).all() and abs(float(loss[0]) - np.log(2.0)) < 1e-6
    assert not logits[:2].any() and (logits[2:] == 5555.0).all()
