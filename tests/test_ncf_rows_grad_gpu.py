"""pmgt_ncf_train_grad_rows -- the NCF head on an item row PER PAIR, the head's half of fine-tuning the encoder -- against
ncf_head_rows_grad_host, by the measure of tests/test_ncf_train_grad_gpu.py (HEADS, NS, C_BOUND and ratios are that file's, imported):

    max|kernel - o64| <= C max(max|r32 - o64|, 2^-22 max|o64|),   C = 4,

per case and per quantity: loss, logits, every gradient tensor of the head and d_item [n, d], the gradient of the item rows.  o64 is the
yardstick in float64, r32 the same in float32.  Every head of HEADS x every n of NS x the three label sets on RANDOM x_item; gradient
buffers and d_item start as NaN and none may survive in what the call owns (rows of d_item past n must still hold it); embedding rows no
pair touches are exactly +0.0.  With x_item = table[items] the call has THE BITS of pmgt_ncf_train_grad_table in loss, logits and the whole
gradient buffer, and d_item summed per item in pair order is that entry's table gradient within the measure.  Dropout (p_emb 0.25,
p_layer 0.5, n = 130) against the yardstick under ncf_dropout_masks; all p = 0 with a non-NULL drop: the bits of the call without.

THE ITEM ROWS ARE CHOSEN WELL-CONDITIONED, on the host alone, by the rule of tests/test_ncf_dropout_grad_gpu.py (which states why: the
gradient is discontinuous where a pre-activation crosses 0, and 130 random rows x every layer meet an element inside its own fp32 error
now and then): a row of x_item is drawn again, from the same generator, until under no masks and under the masks of the dropout case
|a64| > 8 max|a32 - a64| holds on the whole row of every layer.  A property of the reference and its own fp32 error, decided before the
device computes anything.

Measured on the MI355X (one run), the largest ratio of any quantity per head, in HEADS' order: 1.02, 1.01, 1.25, 1.74, 2.71, 2.70 without
dropout (d_item alone: 0.72, 0.78, 1.25, 1.28, 1.28, 1.55) and 0.60, 0.91, 1.24, 1.21, 1.59, 1.49 under the masks; d_item summed per item
0.45, 0.94, 0.70, 0.92, 0.96, 1.26, with the bits of the table entry's own gradient.  Two item rows were drawn again (heads 3 and 5)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.finetune import NcfRowsGrad
from pmgt_amd.ncf_head import TABLE_KEY, head_layout, ncf_dropout_masks, ncf_head_grad_host, ncf_head_rows_grad_host
from pmgt_amd.ncf_train import NcfDropoutC, NcfHeadGrad, NcfTrainC
from tests.test_ncf_train_grad_gpu import C_BOUND, HEADS, ITEM_NUM, NS, USER_NUM, flatten, ratios
from tests.test_recommend_cpu import random_head

pytestmark = pytest.mark.gpu

SEED, STEP, P_EMB, P_LAYER = 0x1234_5678_9ABC, 3, 0.25, 0.5
N = NS[-1]


def pre_activations(w, x_item, users, masks, dtype):
    """[a_0, .., a_(L-1)]: W_l h_l + b_l of the head on the rows x_item under `masks` (None: none), before the layer's mask and the ReLU"""
    m = {} if masks is None else {k: keep.astype(dtype) * dtype(scale) for k, (keep, scale) in masks.items()}
    h = np.concatenate([w["mlp_user_embeddings.weight"][users], x_item], axis=1).astype(dtype) * m.get("emb", dtype(1))
    out, i = [], 0
    while f"mlp_layers.{i}.linear.weight" in w:
        out.append(h @ w[f"mlp_layers.{i}.linear.weight"].astype(dtype).T + w[f"mlp_layers.{i}.linear.bias"].astype(dtype))
        h = np.maximum(out[-1] * m.get(f"layer{i}", dtype(1)), 0)
        i += 1
    return out


def ill_conditioned_rows(shape, w, x_item, users):
    bad = np.zeros(len(users), dtype=bool)
    for masks in (None, ncf_dropout_masks(SEED, STEP, len(users), *shape, P_EMB, P_LAYER)):
        for a64, a32 in zip(pre_activations(w, x_item, users, masks, np.float64), pre_activations(w, x_item, users, masks, np.float32)):
            bad |= ~(np.abs(a64).min(axis=1) > 8 * np.abs(a32 - a64).max())
    return bad


@functools.lru_cache(maxsize=None)
def world(shape):
    w, table = random_head(*shape, USER_NUM, ITEM_NUM, seed=4000 + 10 * shape[0] + shape[1])
    layout, count = head_layout(*shape, USER_NUM, ITEM_NUM)
    rng = np.random.default_rng(31)
    users, items = rng.integers(0, USER_NUM - 1, size=N), rng.integers(0, ITEM_NUM - 1, size=N)      # user 4 and item 6 never appear
    mixed = (rng.random(N) < 0.4).astype(np.float32)
    x = rng.standard_normal((N, table.shape[1])).astype(np.float32)
    for _ in range(64):
        bad = np.nonzero(ill_conditioned_rows(shape, w, x, users))[0]
        if len(bad) == 0:
            break
        print(f"head {shape}: item rows {bad.tolist()} drawn again")
        x[bad] = rng.standard_normal((len(bad), x.shape[1])).astype(np.float32)
    else:
        raise AssertionError(f"no well-conditioned item rows for head {shape}")
    return dict(shape=shape, w=w, table=table, layout=layout, count=count, users=users, items=items, mixed=mixed, x=x,
                flat=torch.from_numpy(flatten(w, layout, count)).cuda())


@pytest.fixture(scope="module", params=HEADS, ids=lambda h: f"f{h[0]}-L{h[1]}-{h[2]}")
def head(request):
    return world(request.param)


def make_fn(h, x_item, dropout=None):
    """An NcfRowsGrad over the world's parameters with buffers of its own: grads, x_item [N, d] and d_item [N, d]"""
    nan = lambda *size: torch.full(size, float("nan"), device="cuda")
    fn = NcfRowsGrad(*h["shape"], USER_NUM, ITEM_NUM, h["flat"], nan(h["count"]), dropout=dropout)
    fn.bind(torch.from_numpy(np.ascontiguousarray(x_item)).cuda(), nan(N, x_item.shape[1]))
    return fn


def run(fn, users, items, labels):
    fn.grads.fill_(float("nan"))                             # written whole: no NaN may survive
    fn.d_item.fill_(float("nan"))
    loss, logits = fn(torch.from_numpy(users).cuda(), torch.from_numpy(items).cuda(), torch.from_numpy(labels).cuda())
    return loss.clone(), logits.clone(), fn.grads.clone(), fn.d_item.clone()


def split(raw, layout, n):
    loss, logits, grads, d_item = raw
    g, di = grads.cpu().numpy(), d_item.cpu().numpy()
    assert np.isnan(di[n:]).all()                            # rows past n are not the call's
    out = {"loss": loss.cpu().numpy(), "logits": logits.cpu().numpy(), "d_item": di[:n]}
    out.update({k: g[off: off + int(np.prod(shape))].reshape(shape) for k, (off, shape) in layout.items()})
    return out


def host(h, x_item, users, items, labels, dtype, masks=None):
    loss, logits, grads, d_item = ncf_head_rows_grad_host(h["w"], x_item, users, items, labels, dtype, masks=masks)
    return dict(grads, loss=np.asarray([loss]), logits=logits, d_item=d_item)


def check_case(h, fn, n, labels, what, masks=None):
    users, items, x = h["users"][:n], h["items"][:n], h["x"][:n]
    got = split(run(fn, users, items, labels), h["layout"], n)
    o64, r32 = host(h, x, users, items, labels, np.float64, masks), host(h, x, users, items, labels, np.float32, masks)
    assert all(np.isfinite(v).all() for v in got.values()), what
    rt = ratios(got, o64, r32)
    print(f"head {h['shape']} {what}: " + ", ".join(f"{k} {v:.2f}" for k, v in rt.items()))
    for k in [k for k in got if "embeddings" in k]:          # untouched rows: exactly +0.0
        idx = items if k.startswith("gmf_item") else users
        untouched = np.setdiff1d(np.arange(len(got[k])), idx)
        assert len(untouched) >= 1 and (got[k][untouched].view(np.uint32) == 0).all(), (what, k)
    bad = {k: v for k, v in rt.items() if not v <= C_BOUND}
    assert not bad, (h["shape"], what, bad)
    return rt


def test_loss_logits_every_gradient_and_d_item_within_the_bound(head):
    fn, worst = make_fn(head, head["x"]), {}
    for n in NS:
        for name, labels in (("mixed", head["mixed"][:n]), ("zeros", np.zeros(n, np.float32)), ("ones", np.ones(n, np.float32))):
            for k, v in check_case(head, fn, n, labels, f"n {n} labels {name}").items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(f"head {head['shape']}: largest ratios " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


def test_on_table_rows_the_bits_of_the_table_entry(head):
    h, n = head, N
    users, items, labels = h["users"], h["items"], h["mixed"]
    table_d = torch.from_numpy(h["table"]).cuda()
    nan = lambda *size: torch.full(size, float("nan"), device="cuda")
    tfn = NcfHeadGrad(*h["shape"], USER_NUM, table_d, h["flat"], nan(h["count"]), table_grad=nan(*h["table"].shape))
    args = [torch.from_numpy(a).cuda() for a in (users, items, labels)]
    t_loss, t_logits = tfn(*args)
    loss, logits, grads, d_item = run(make_fn(h, h["table"][items]), users, items, labels)
    assert torch.equal(loss, t_loss) and torch.equal(logits, t_logits) and torch.equal(grads, tfn.grads)
    # d_item summed per item IN PAIR ORDER (np.add.at adds in index order) against the yardstick's table gradient, the kernel's own next to it
    summed = np.zeros_like(h["table"])
    np.add.at(summed, items, d_item.cpu().numpy())
    o64 = ncf_head_grad_host(h["w"], h["table"], users, items, labels, np.float64, table_grad=True)[2][TABLE_KEY]
    r32 = ncf_head_grad_host(h["w"], h["table"], users, items, labels, np.float32, table_grad=True)[2][TABLE_KEY]
    rt = ratios({"summed": summed, "table_grad": tfn.table_grad.cpu().numpy()}, {"summed": o64, "table_grad": o64}, {"summed": r32, "table_grad": r32})
    print(f"head {h['shape']}: d_item summed per item {rt['summed']:.2f}, the table entry's own {rt['table_grad']:.2f}")
    assert rt["summed"] <= C_BOUND, rt
    assert np.array_equal(summed, tfn.table_grad.cpu().numpy())      # (the same rows added in the same order: in fact the same bits)


def test_dropout_against_the_yardstick_under_the_host_masks(head):
    shape = head["shape"]
    rng = torch.tensor([SEED, STEP], dtype=torch.int64, device="cuda")
    masks = ncf_dropout_masks(SEED, STEP, N, *shape, P_EMB, P_LAYER)
    fn = make_fn(head, head["x"], dropout=(rng, P_EMB, P_LAYER))
    check_case(head, fn, N, head["mixed"], f"dropout p_emb {P_EMB} p_layer {P_LAYER}", masks=masks)
    d_item = fn.d_item.cpu().numpy()
    keep = masks["emb"][0][:, head["x"].shape[1]:]
    assert not keep.all() and not d_item[~keep].any()        # d_item carries the emb mask


def test_all_p_zero_with_a_drop_gives_the_bits_of_no_dropout(head):
    rng = torch.tensor([SEED, STEP], dtype=torch.int64, device="cuda")
    a = run(make_fn(head, head["x"]), head["users"], head["items"], head["mixed"])
    b = run(make_fn(head, head["x"], dropout=(rng, 0.0, 0.0)), head["users"], head["items"], head["mixed"])
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_the_same_inputs_give_the_same_bits(head):
    fn = make_fn(head, head["x"])
    a = run(fn, head["users"], head["items"], head["mixed"])
    b = run(fn, head["users"], head["items"], head["mixed"])
    c = run(make_fn(head, head["x"]), head["users"], head["items"], head["mixed"])      # other buffers, another workspace
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_refused_before_any_launch():
    lib = _lib.hip()
    buf = torch.zeros(1 << 16, device="cuda")                # parameters, item rows and labels: zeros
    work, loss = torch.zeros(1 << 12, device="cuda"), torch.zeros(1, device="cuda")
    ids = torch.zeros(64, dtype=torch.int64, device="cuda")
    canary, canary2 = torch.full((4096,), float("nan"), device="cuda"), torch.full((4096,), float("nan"), device="cuda")
    rng = torch.zeros(2, dtype=torch.int64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    need = int(lib.pmgt_ncf_train_rows_workspace_bytes(8, 2, 0, 2))
    assert need > 0 and need == int(lib.pmgt_ncf_train_table_workspace_bytes(8, 2, 0, 2))

    def call(factor=8, num_layers=2, kind=0, n=2, x_item=buf.data_ptr(), d_item=canary2.data_ptr(), params=buf.data_ptr(),
             grads=canary.data_ptr(), users=ids.data_ptr(), ws=work.data_ptr(), ws_bytes=need, user_num=2, item_num=2, drop=None):
        h = NcfTrainC()
        h.factor_num, h.num_layers, h.kind, h.user_num, h.item_num = factor, num_layers, kind, user_num, item_num
        h.table, h.params, h.grads = None, params, grads     # the table is not read: NULL is fine
        d = None
        if drop is not None:
            d = NcfDropoutC(drop.get("rng", rng.data_ptr()), drop.get("p_emb", 0.0))
            for i in range(4):
                d.p_layer[i] = drop.get("p_layer", 0.0)
        return lib.pmgt_ncf_train_grad_rows(C.byref(h), users, ids.data_ptr(), buf.data_ptr(), n, loss.data_ptr(), None, x_item, d_item,
                                            None if d is None else C.byref(d), ws, ws_bytes, st)

    bad = [dict(factor=12), dict(factor=128), dict(num_layers=0), dict(num_layers=5), dict(factor=64, num_layers=4), dict(kind=2), dict(n=0),
           dict(n=65537), dict(params=0), dict(grads=0), dict(users=0), dict(ws=0), dict(ws_bytes=need - 4),
           dict(grads=canary.data_ptr() + 8), dict(user_num=0), dict(item_num=0),
           dict(x_item=0), dict(d_item=0), dict(x_item=buf.data_ptr() + 4), dict(d_item=canary2.data_ptr() + 8),
           dict(drop=dict(p_emb=1.0)), dict(drop=dict(p_emb=float("nan"))), dict(drop=dict(p_layer=-0.1)), dict(drop=dict(p_emb=0.5, rng=None)),
           dict(drop=dict(p_layer=0.5, rng=rng.data_ptr() + 4))]
    assert [call(**b) for b in bad] == [-2] * len(bad)
    assert lib.pmgt_ncf_train_rows_workspace_bytes(8, 2, 0, 0) == -2 and lib.pmgt_ncf_train_rows_workspace_bytes(8, 2, 0, 65537) == -2
    torch.cuda.synchronize()
    assert torch.isnan(canary).all() and torch.isnan(canary2).all()      # nothing was launched
    assert call() == 0 and call(drop={}) == 0                # all-zero parameters: logits 0, loss log 2, d_item 0
    torch.cuda.synchronize()
    count = int(lib.pmgt_ncf_train_layout(8, 2, 0, 2, 2, None))
    assert torch.isnan(canary[count:]).all() and not torch.isnan(canary[:count]).any() and abs(float(loss[0]) - np.log(2.0)) < 1e-6
    assert torch.isnan(canary2[2 * 16:]).all() and (canary2[:2 * 16] == 0).all()
