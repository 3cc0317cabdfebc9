"""pmgt_ncf_train_grad_table on synthetic heads: the gradient of the item table next to everything pmgt_ncf_train_grad gives, by the measure
of tests/test_ncf_train_grad_gpu.py.

Per case and per quantity (loss, logits, the head's gradient tensors and item_table), o64 = ncf_head_grad_host(..., np.float64,
table_grad=True), r32 = the same in np.float32:
    max|kernel - o64| <= C max(max|r32 - o64|, 2^-22 max|o64|),   C = 4.
The table's gradient is the other column half of the product that gives mlp_user_embeddings (W_0^T dz_0, columns d .. 2 d), summed over the
runs of equal item ids in pair order, so its error class is that tensor's.  Loss, logits and the head's thirteen tensors must have THE BITS
of pmgt_ncf_train_grad on the same inputs: the wider product computes every column block on its own.  user_num = 5 and I = 7 with pairs drawn
from 4 users x 6 items: duplicates are forced, user 4 and item 6 never appear and their rows -- item 6's row of the table gradient too --
must be exactly +0.0; every gradient buffer is pre-filled with NaN and none may survive.
Measured on the MI355X (one run): the largest ratio of item_table per head 0.79, 1.34, 1.15, 2.34, 1.79, 1.74 (mlp_user_embeddings: 1.97 at most);
one run of 130 pairs 1.16 and 0.94, descending ids 0.92 and 0.92; at 65 536 pairs 0.89."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from pmgt_amd.ncf_train import TABLE_KEY, NcfHeadGrad, NcfTrainC, head_layout, ncf_head_grad_host
from tests.test_ncf_train_grad_gpu import C_BOUND, HEADS, ITEM_NUM, NS, USER_NUM, flatten, ratios
from tests.test_recommend_cpu import random_head

pytestmark = pytest.mark.gpu


def device_grads(w, table, shape, user_num):
    """(the entry with the table trained, the entry with it frozen, the head's layout): each over buffers of its own, NaN-filled"""
    layout, count = head_layout(*shape, user_num, len(table))
    flat = torch.from_numpy(flatten(w, layout, count)).cuda()
    table_d = torch.from_numpy(table).cuda()
    nan = lambda *size: torch.full(size, float("nan"), device="cuda")
    trained = NcfHeadGrad(*shape, user_num, table_d, flat, nan(count), table_grad=nan(*table.shape))
    frozen = NcfHeadGrad(*shape, user_num, table_d.clone(), flat.clone(), nan(count))
    return trained, frozen, layout


def run(fn, users, items, labels):
    fn.grads.fill_(float("nan"))                             # both buffers are written whole: no NaN may survive
    if fn.table_grad is not None:
        fn.table_grad.fill_(float("nan"))
    loss, logits = fn(torch.from_numpy(users).cuda(), torch.from_numpy(items).cuda(), torch.from_numpy(labels).cuda())
    return loss.clone(), logits.clone(), fn.grads.clone(), None if fn.table_grad is None else fn.table_grad.clone()


def split(loss, logits, grads, table_grad, layout):
    g = grads.cpu().numpy()
    out = {"loss": loss.cpu().numpy(), "logits": logits.cpu().numpy(), TABLE_KEY: table_grad.cpu().numpy()}
    out.update({k: g[off: off + int(np.prod(shape))].reshape(shape) for k, (off, shape) in layout.items()})
    return out


def host(w, table, users, items, labels, dtype):
    loss, logits, grads = ncf_head_grad_host(w, table, users, items, labels, dtype, table_grad=True)
    return dict(grads, loss=np.asarray([loss]), logits=logits)


@functools.lru_cache(maxsize=None)
def world(shape):
    factor, num_layers, kind = shape
    w, table = random_head(factor, num_layers, kind, USER_NUM, ITEM_NUM, seed=2000 + 10 * factor + num_layers)
    rng = np.random.default_rng(17)
    users, items = rng.integers(0, USER_NUM - 1, size=NS[-1]), rng.integers(0, ITEM_NUM - 1, size=NS[-1])
    mixed = (rng.random(NS[-1]) < 0.4).astype(np.float32)
    trained, frozen, layout = device_grads(w, table, shape, USER_NUM)
    return dict(shape=shape, w=w, table=table, users=users, items=items, mixed=mixed, trained=trained, frozen=frozen, layout=layout)


@pytest.fixture(scope="module", params=HEADS, ids=lambda h: f"f{h[0]}-L{h[1]}-{h[2]}")
def head(request):
    return world(request.param)


def check_case(h, users, items, labels, what, items_left_out=True):
    raw = run(h["trained"], users, items, labels)
    got = split(*raw, h["layout"])
    o64, r32 = host(h["w"], h["table"], users, items, labels, np.float64), host(h["w"], h["table"], users, items, labels, np.float32)
    assert sorted(got) == sorted(o64) and all(np.isfinite(v).all() for v in got.values()), what
    rt = ratios(got, o64, r32)
    print(f"head {h['shape']} {what}: " + ", ".join(f"{k} {v:.2f}" for k, v in rt.items()))
    for k in [k for k in got if "embeddings" in k or k == TABLE_KEY]:      # untouched rows: exactly +0.0
        by_item = k.startswith("gmf_item") or k == TABLE_KEY
        untouched = np.setdiff1d(np.arange(len(got[k])), items if by_item else users)
        assert len(untouched) >= (1 if items_left_out or not by_item else 0) and (got[k][untouched].view(np.uint32) == 0).all(), (what, k)
    touched = np.unique(items)
    assert got[TABLE_KEY][touched].any(axis=1).all(), what   # (a seeded head: no touched row has a gradient of zero)
    bad = {k: v for k, v in rt.items() if not v <= C_BOUND}
    assert not bad, (h["shape"], what, bad)
    # loss, logits and the whole gradient buffer of the head: the bits of the entry that leaves the table frozen
    ref = run(h["frozen"], users, items, labels)
    assert all(torch.equal(a, b) for a, b in zip(raw[:3], ref[:3])), (h["shape"], what)
    return rt


def test_the_table_gradient_and_everything_else_within_the_bound(head):
    worst = {}
    for n in NS:
        for name, labels in (("mixed", head["mixed"][:n]), ("zeros", np.zeros(n, np.float32)), ("ones", np.ones(n, np.float32))):
            rt = check_case(head, head["users"][:n], head["items"][:n], labels, f"n {n} labels {name}")
            for k, v in rt.items():
                worst[k] = max(worst.get(k, 0.0), v)
    print(f"head {head['shape']}: largest ratios " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


@pytest.mark.parametrize("shape", [(8, 1, "MLP"), (64, 3, "NeuMF-end")], ids=lambda h: f"f{h[0]}-L{h[1]}-{h[2]}")
def test_one_long_run_and_the_stable_order_against_the_pair_order(shape):
    """d = 8: both widths of the data gradient sit below one 32-block; d = 256: the item half is column blocks 8 .. 15."""
    h, n = world(shape), 130
    check_case(h, h["users"][:n], np.full(n, 3, dtype=np.int64), h["mixed"][:n], "every pair on item 3")
    descending = (ITEM_NUM - 1 - np.arange(n) % ITEM_NUM).astype(np.int64)      # 6, 5, .., 0, 6, ..: the stable order reverses the pairs
    check_case(h, h["users"][:n], descending, h["mixed"][:n], "item ids descending", items_left_out=False)


def test_the_same_inputs_give_the_same_bits(head):
    n = 130
    args = (head["users"][:n], head["items"][:n], head["mixed"][:n])
    a, b = run(head["trained"], *args), run(head["trained"], *args)
    other, _, _ = device_grads(head["w"], head["table"], head["shape"], USER_NUM)      # other buffers, another workspace
    c = run(other, *args)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)


def test_the_most_pairs_one_call_takes():
    """65 536 pairs: item_table is a sum over short runs (13 pairs an item on average), judged like the per-row quantities; the sums over
    all pairs are judged in tests/test_ncf_train_grad_gpu.py, here they must have the frozen entry's bits."""
    from pmgt_amd.ncf_train import NCF_TRAIN_MAX_PAIRS
    shape, user_num, item_num, n = (8, 2, "NeuMF-end"), 3000, 5000, NCF_TRAIN_MAX_PAIRS
    w, table = random_head(*shape, user_num, item_num, seed=5)
    rng = np.random.default_rng(23)
    users, items = rng.integers(1, user_num, size=n), rng.integers(0, item_num - 1, size=n)
    labels = (rng.random(n) < 0.3).astype(np.float32)
    trained, frozen, layout = device_grads(w, table, shape, user_num)
    raw = run(trained, users, items, labels)
    got = split(*raw, layout)
    o64, r32 = host(w, table, users, items, labels, np.float64), host(w, table, users, items, labels, np.float32)
    assert all(np.isfinite(v).all() for v in got.values())
    untouched = np.setdiff1d(np.arange(item_num), items)
    assert item_num - 1 in untouched and (got[TABLE_KEY][untouched].view(np.uint32) == 0).all()
    rt = ratios(got, o64, r32)
    print("65536 pairs: " + ", ".join(f"{k} {v:.2f}" for k, v in rt.items()))
    per_row = [k for k in got if "embeddings" in k or k in (TABLE_KEY, "logits")]
    bad = {k: rt[k] for k in per_row if not rt[k] <= C_BOUND}
    assert TABLE_KEY in per_row and not bad, bad
    ref = run(frozen, users, items, labels)
    assert all(torch.equal(a, b) for a, b in zip(raw[:3], ref[:3]))
    with pytest.raises(ValueError, match="outside"):
        trained.reserve(n + 1)


def test_refused_before_any_launch():
    from pmgt_amd import _lib
    lib = _lib.hip()
    buf = torch.zeros(1 << 16, device="cuda")                # table, parameters and labels: zeros
    work, loss = torch.zeros(1 << 12, device="cuda"), torch.zeros(1, device="cuda")
    ids = torch.zeros(64, dtype=torch.int64, device="cuda")
    canary, canary_t = torch.full((4096,), 7777.0, device="cuda"), torch.full((4096,), 5555.0, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    need, need_frozen = int(lib.pmgt_ncf_train_table_workspace_bytes(8, 2, 0, 2)), int(lib.pmgt_ncf_train_workspace_bytes(8, 2, 0, 2))
    assert need == need_frozen + 2 * 16 * 4 and need <= work.numel() * 4      # one more row [d = 16] per pair

    def call(factor=8, num_layers=2, kind=0, n=2, table=buf.data_ptr(), params=buf.data_ptr(), grads=canary.data_ptr(), users=ids.data_ptr(),
             table_grad=canary_t.data_ptr(), ws=work.data_ptr(), ws_bytes=need, user_num=2, item_num=2):
        h = NcfTrainC()
        h.factor_num, h.num_layers, h.kind, h.user_num, h.item_num = factor, num_layers, kind, user_num, item_num
        h.table, h.params, h.grads = table, params, grads
        return lib.pmgt_ncf_train_grad_table(C.byref(h), users, ids.data_ptr(), buf.data_ptr(), n, loss.data_ptr(), 0, table_grad, ws, ws_bytes, st)

    bad = [dict(factor=12), dict(factor=128), dict(num_layers=0), dict(num_layers=5), dict(factor=64, num_layers=4), dict(kind=2), dict(n=0),
           dict(n=65537), dict(table=0), dict(params=0), dict(grads=0), dict(users=0), dict(ws=0), dict(ws_bytes=need - 4),
           dict(ws_bytes=need_frozen), dict(table=buf.data_ptr() + 4), dict(grads=canary.data_ptr() + 8), dict(user_num=0), dict(item_num=0),
           dict(table_grad=0), dict(table_grad=canary_t.data_ptr() + 4), dict(table_grad=canary_t.data_ptr() + 8)]
    assert [call(**b) for b in bad] == [-2] * len(bad)
    assert lib.pmgt_ncf_train_table_workspace_bytes(8, 2, 0, 0) == -2 and lib.pmgt_ncf_train_table_workspace_bytes(8, 2, 0, 65537) == -2
    assert lib.pmgt_ncf_train_table_workspace_bytes(12, 2, 0, 2) == -2
    torch.cuda.synchronize()
    assert (canary == 7777.0).all() and (canary_t == 5555.0).all()
    assert call() == 0                                       # all-zero parameters: logits 0, loss log 2, a table gradient of zeros
    torch.cuda.synchronize()
    count = int(lib.pmgt_ncf_train_layout(8, 2, 0, 2, 2, None))
    assert (canary[count:] == 7777.0).all() and abs(float(loss[0]) - np.log(2.0)) < 1e-6
    assert not canary_t[:2 * 16].any() and (canary_t[2 * 16:] == 5555.0).all()
