"""NcfHeadTrainer(train_table=True): the step against pmgt_ncf_train_grad_table followed by pmgt_op_adamw over the whole buffer by hand, the
loss trajectory against the torch procedure with the table as a trained parameter in fp64, captured against eager steps, resume from the
state dict, the frozen and the trained state refusing each other, and trainer.table as the view of the buffer that the readers read."""
import ctypes as C

import numpy as np
import pytest
import torch

from pmgt_amd.ncf_train import TABLE_KEY, NcfHeadGrad, NcfHeadTrainer
from tests.ncf_table_util import TorchTableHead
from tests.ncf_train_util import make_model
from tests.test_ncf_train_step_gpu import C_BOUND, HEADS, HYPER, ITEM_NUM, USER_NUM, batches, dev

pytestmark = pytest.mark.gpu


def fresh(shape, clip=5.0, seed=9, table=None, train_table=True, **hyper):
    """(trainer, model, initial weights, initial table) with the head and -- unless one is given -- the table drawn from `seed`"""
    model, w, own = make_model(*shape, USER_NUM, ITEM_NUM, seed)
    table = own if table is None else table
    tr = NcfHeadTrainer(model, torch.from_numpy(table).cuda(), max_grad_norm=clip, train_table=train_table, **{**HYPER, **hyper})
    return tr, model, w, table


def pad_of(tr):
    """[the end of the head, the start of the table) in floats: the pad"""
    return sum(int(np.prod(s)) for k, (_, s) in tr.layout.items() if k != TABLE_KEY), tr.layout[TABLE_KEY][0]


@pytest.mark.parametrize("clip", [None, 0.05], ids=["no-clip", "clip"])
@pytest.mark.parametrize("shape", HEADS, ids=lambda h: f"f{h[0]}-L{h[1]}-{h[2]}")
def test_step_is_the_table_gradient_entry_then_adamw_over_the_whole_buffer(shape, clip):
    from pmgt_amd import _lib
    tr, model, w, table = fresh(shape, clip)
    lo, hi = pad_of(tr)
    assert hi % 8 == 0 and 0 < hi - lo < 8 and tr.count == hi + ITEM_NUM * table.shape[1]
    b = dev(batches(1, 77)[0])
    p = tr.params.clone()
    g = torch.full_like(p, float("nan"))
    g[lo:hi] = 0                                             # the pad: written by nobody, zero from the start
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step, scal, part = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(8, device="cuda"), torch.zeros(1024, device="cuda")
    n_table = ITEM_NUM * table.shape[1]
    loss_hand, _ = NcfHeadGrad(*shape, USER_NUM, p[hi: hi + n_table].view(table.shape), p[:lo], g[:lo],
                               table_grad=g[hi: hi + n_table].view(table.shape))(*b)
    _lib.check(_lib.hip().pmgt_op_adamw(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), tr.decay.data_ptr(), p.numel(), HYPER["lr"],
                                        HYPER["weight_decay"], 0.9, 0.999, 1e-8, clip or 0.0, step.data_ptr(), scal.data_ptr(), part.data_ptr(),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    before = tr.params.clone()
    loss = tr.step(*b)
    assert torch.equal(loss, loss_hand) and torch.equal(tr.grads, g) and bool(torch.isfinite(g).all())
    assert torch.equal(tr.params, p) and torch.equal(tr.exp_avg, m) and torch.equal(tr.exp_avg_sq, v) and int(tr.step_count) == 1
    assert not torch.equal(tr.params[:lo], before[:lo]) and not torch.equal(tr.params[hi:], before[hi:])      # head and table both moved
    norm = float(scal[3])
    assert (float(scal[0]) < 1.0) == (clip is not None and norm > clip), (norm, float(scal[0]))      # the clip case does clip
    # ONE global norm over head and table
    gd = g.double()
    assert abs(norm - float(gd.square().sum().sqrt())) <= 1e-5 * norm and float(gd[hi:].square().sum()) > 0
    # the decay mask: weights, embeddings and the table, not the biases; the pad is outside every view and 0 everywhere
    mask = tr.views(tr.decay)
    assert TABLE_KEY in mask and all(bool(t.all()) != k.endswith(".bias") and bool(t.any()) != k.endswith(".bias") for k, t in mask.items())
    for name in ("params", "grads", "exp_avg", "exp_avg_sq", "decay"):
        assert not getattr(tr, name)[lo:hi].any(), name


@pytest.mark.parametrize("shape", HEADS, ids=lambda h: f"f{h[0]}-L{h[1]}-{h[2]}")
def test_loss_trajectory_against_the_torch_procedure_with_a_trained_table(shape):
    """20 steps on fixed batches: per-step loss of the device trainer against autograd + clip_grad_norm_ + AdamW in fp64 torch on the CPU
    with the table as one more parameter, the same procedure in fp32 torch as the measure:
    max|dev - o64| <= C max(max|r32 - o64|, 2^-22 max|o64|), C = 4.  Measured on the MI355X (one run): ratio 0.65 for (16, 3, NeuMF-end), 0.72
    for (32, 3, MLP); the table moved by up to 0.165 and 0.146."""
    tr, model, w, table = fresh(shape, clip=5.0)
    bs = batches(20, 96)
    got = torch.stack([tr.step(*dev(b)).clone() for b in bs]).view(-1).cpu().numpy().astype(np.float64)
    o64 = TorchTableHead(w, table, torch.float64, max_grad_norm=5.0, **HYPER)
    r32 = TorchTableHead(w, table, torch.float32, max_grad_norm=5.0, **HYPER)
    l64, l32 = np.array([o64.step(*b) for b in bs]), np.array([r32.step(*b) for b in bs])
    scale = max(np.abs(l32 - l64).max(), 2.0 ** -22 * np.abs(l64).max())
    ratio = np.abs(got - l64).max() / scale
    moved = np.abs(tr.table.cpu().numpy() - table).max()
    print(f"head {shape}: loss {l64[0]:.4f} -> {l64[-1]:.4f}; device error {np.abs(got - l64).max():.3e}, fp32 torch error "
          f"{np.abs(l32 - l64).max():.3e}, ratio {ratio:.2f}; the table moved by up to {moved:.3f}")
    assert l64[-1] < l64[0] and moved > 1e-2                 # the procedure learns on these batches; the table moved by more than one lr
    assert ratio <= C_BOUND, ratio


@pytest.mark.parametrize("shape", HEADS, ids=lambda h: f"f{h[0]}-L{h[1]}-{h[2]}")
def test_replayed_steps_equal_eager_steps(shape):
    bs = batches(3, 130)
    eager, _, _, _ = fresh(shape)
    losses_e = [eager.step(*dev(b)).clone() for b in bs]
    graph, _, _, _ = fresh(shape)
    start = graph.params.clone()
    users, items, labels, loss = graph.capture(130)
    assert torch.equal(graph.params, start) and int(graph.step_count) == 0 and not graph.exp_avg.any()      # capturing moved nothing
    losses_g = []
    for b in bs:
        for dst, src in zip((users, items, labels), dev(b)):
            dst.copy_(src)
        losses_g.append(graph.replay().clone())
    for a, b in zip(losses_e, losses_g):
        assert torch.equal(a, b)
    for name in ("params", "exp_avg", "exp_avg_sq", "step_count", "grads", "table"):
        assert torch.equal(getattr(eager, name), getattr(graph, name)), name
    assert int(graph.step_count) == 3


def test_resume_from_the_state_dict_and_the_two_kinds_of_state():
    shape = HEADS[0]
    bs = batches(6, 64)
    straight, _, _, _ = fresh(shape)
    for b in bs:
        straight.step(*dev(b))
    first, _, _, table = fresh(shape)
    for b in bs[:3]:
        first.step(*dev(b))
    sd = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in first.state_dict().items()}
    assert TABLE_KEY in sd["layout"]
    second, _, _, _ = fresh(shape, seed=10)                  # other initial weights and another initial table: all of it comes from the state
    second.load_state_dict(sd)
    for b in bs[3:]:
        second.step(*dev(b))
    for name in ("params", "exp_avg", "exp_avg_sq", "step_count", "table"):
        assert torch.equal(getattr(straight, name), getattr(second, name)), name
    assert int(second.step_count) == 6
    frozen, _, _, _ = fresh(shape, train_table=False)
    assert TABLE_KEY not in frozen.state_dict()["layout"]
    with pytest.raises(ValueError, match="layouts differ"):
        frozen.load_state_dict(sd)
    with pytest.raises(ValueError, match="layouts differ"):
        second.load_state_dict(frozen.state_dict())


def test_the_table_is_a_view_that_moves_where_items_appeared_and_the_readers_read_it():
    from pmgt_amd.evaluation import rank_users
    from pmgt_amd.recommend import host_scores, ncf_head_host, recommend
    from pmgt_amd.ncf_train import head_state
    shape = HEADS[0]
    tr, model, w, table = fresh(shape, weight_decay=0.0)     # no decay: a row without a gradient keeps its bits
    lo, hi = tr.params.data_ptr(), tr.params.data_ptr() + 4 * tr.params.numel()
    assert lo < tr.table.data_ptr() < hi and tr.table.data_ptr() == lo + 4 * tr.layout[TABLE_KEY][0] and tr.table.data_ptr() % 32 == 0
    assert tr.table.untyped_storage().data_ptr() == tr.params.untyped_storage().data_ptr()
    assert np.array_equal(tr.table.cpu().numpy(), table) and tuple(tr.table.shape) == table.shape
    users, items, labels = batches(1, 64)[0]
    items = items % 29                                       # items 29 .. 40 do not appear
    tr.step(*dev((users, items, labels)))
    changed = np.nonzero((tr.table.cpu().numpy().view(np.uint32) != table.view(np.uint32)).any(axis=1))[0]
    assert np.array_equal(changed, np.unique(items)) and len(changed) < ITEM_NUM
    # the readers: model.head through rank_users and recommend over trainer.table, against the fp64 formula on the trained head and table
    now = {k: v.detach().cpu().numpy() for k, v in head_state(model).items()}
    all_users = np.arange(USER_NUM)
    model.eval()
    o64 = ncf_head_host(now, all_users, tr.table.cpu().numpy(), np.float64)
    s_h = host_scores(model, tr.table, all_users)
    tol = 4 * max(np.abs(s_h - o64).max(), 2.0 ** -22 * np.abs(o64).max())
    assert np.abs(s_h - ncf_head_host(now, all_users, table, np.float64)).max() > 1e3 * tol      # not the initial table
    top, scores = recommend(model, None, all_users, k=5, table=tr.table)
    assert np.abs(scores.astype(np.float64) - np.take_along_axis(s_h, top, axis=1)).max() <= tol
    cand = torch.arange(ITEM_NUM, device="cuda").repeat(USER_NUM, 1)
    rows = []
    rank_users(model, tr.table, torch.from_numpy(all_users).cuda(), cand, torch.zeros(USER_NUM, ITEM_NUM, device="cuda"),
               torch.full((USER_NUM,), ITEM_NUM, dtype=torch.int32, device="cuda"), sink=lambda lg, lb, ct, at: rows.append(lg.clone()))
    assert np.abs(torch.cat(rows).cpu().numpy().astype(np.float64) - s_h).max() <= tol
    # one more step is seen at once: nothing was copied
    tr.step(*dev(batches(1, 64, seed=8)[0]))
    assert np.abs(host_scores(model, tr.table, all_users) - s_h).max() > 0
