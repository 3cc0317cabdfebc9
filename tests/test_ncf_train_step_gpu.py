"""NcfHeadTrainer: the step against its two parts called by hand, the loss trajectory against the torch procedure in fp64, captured against
eager steps, resume from the trainer's state dict, and the model's parameters as views of the trained buffer."""
import ctypes as C

import numpy as np
import pytest
import torch

from pmgt_amd.ncf_train import NcfHeadGrad, NcfHeadTrainer, head_state
from tests.ncf_train_util import TorchHead, make_model

pytestmark = pytest.mark.gpu

USER_NUM, ITEM_NUM = 23, 41
HEADS = [(16, 3, "NeuMF-end"), (32, 3, "MLP")]
HYPER = dict(lr=1e-2, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8)
C_BOUND = 4.0


def batches(count, n, seed=3):
    rng = np.random.default_rng(seed)
    return [(rng.integers(0, USER_NUM, size=n), rng.integers(0, ITEM_NUM, size=n), (rng.random(n) < 0.4).astype(np.float32)) for _ in range(count)]


def dev(batch):
    return tuple(torch.from_numpy(a).cuda() for a in batch)


def fresh(shape, clip=5.0, seed=9, table=None):
    """(trainer, model, initial weights, table) with the head and -- unless one is given -- the frozen table drawn from `seed`"""
    model, w, own = make_model(*shape, USER_NUM, ITEM_NUM, seed)
    table = own if table is None else table
    return NcfHeadTrainer(model, torch.from_numpy(table).cuda(), max_grad_norm=clip, **HYPER), model, w, table


@pytest.mark.parametrize("clip", [None, 0.05], ids=["no-clip", "clip"])
@pytest.mark.parametrize("shape", HEADS, ids=lambda h: f"f{h[0]}-L{h[1]}-{h[2]}")
def test_step_is_the_gradient_entry_then_adamw(shape, clip):
    from pmgt_amd import _lib
    tr, model, w, table = fresh(shape, clip)
    b = dev(batches(1, 77)[0])
    p = tr.params.clone()
    g = torch.full_like(p, float("nan"))
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step, scal, part = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(8, device="cuda"), torch.zeros(1024, device="cuda")
    loss_hand, _ = NcfHeadGrad(*shape, USER_NUM, tr.table, p, g)(*b)
    _lib.check(_lib.hip().pmgt_op_adamw(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), tr.decay.data_ptr(), p.numel(), HYPER["lr"],
                                        HYPER["weight_decay"], 0.9, 0.999, 1e-8, clip or 0.0, step.data_ptr(), scal.data_ptr(), part.data_ptr(),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    before = tr.params.clone()
    loss = tr.step(*b)
    assert torch.equal(loss, loss_hand) and torch.equal(tr.grads, g)
    assert torch.equal(tr.params, p) and torch.equal(tr.exp_avg, m) and torch.equal(tr.exp_avg_sq, v) and int(tr.step_count) == 1
    assert not torch.equal(tr.params, before)
    norm = float(scal[3])
    assert (float(scal[0]) < 1.0) == (clip is not None and norm > clip), (norm, float(scal[0]))      # the clip case does clip
    # the decay mask: weights and embeddings, not biases
    mask = tr.views(tr.decay)
    assert all(bool(t.all()) != k.endswith(".bias") and bool(t.any()) != k.endswith(".bias") for k, t in mask.items())


@pytest.mark.parametrize("shape", HEADS, ids=lambda h: f"f{h[0]}-L{h[1]}-{h[2]}")
def test_loss_trajectory_against_the_torch_procedure(shape):
    """20 steps on fixed batches: per-step loss of the device trainer against autograd + clip_grad_norm_ + AdamW in fp64 torch on the CPU,
    with the same procedure in fp32 torch as the measure: max|dev - o64| <= C max(max|r32 - o64|, 2^-22 max|o64|).  Measured on the MI355X
    (one run): ratio 0.94 for (16, 3, NeuMF-end), 0.73 for (32, 3, MLP)."""
    tr, model, w, table = fresh(shape, clip=5.0)
    bs = batches(20, 96)
    got = torch.stack([tr.step(*dev(b)).clone() for b in bs]).view(-1).cpu().numpy().astype(np.float64)
    o64 = TorchHead(w, table, torch.float64, max_grad_norm=5.0, **HYPER)
    r32 = TorchHead(w, table, torch.float32, max_grad_norm=5.0, **HYPER)
    l64, l32 = np.array([o64.step(*b) for b in bs]), np.array([r32.step(*b) for b in bs])
    scale = max(np.abs(l32 - l64).max(), 2.0 ** -22 * np.abs(l64).max())
    ratio = np.abs(got - l64).max() / scale
    print(f"head {shape}: loss {l64[0]:.4f} -> {l64[-1]:.4f}; device error {np.abs(got - l64).max():.3e}, fp32 torch error "
          f"{np.abs(l32 - l64).max():.3e}, ratio {ratio:.2f}")
    assert l64[-1] < l64[0]                                  # the procedure does learn on these batches
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
    for name in ("params", "exp_avg", "exp_avg_sq", "step_count", "grads"):
        assert torch.equal(getattr(eager, name), getattr(graph, name)), name
    assert int(graph.step_count) == 3


def test_resume_from_the_state_dict():
    shape = HEADS[0]
    bs = batches(6, 64)
    straight, _, _, _ = fresh(shape)
    for b in bs:
        straight.step(*dev(b))
    first, _, _, table = fresh(shape)
    for b in bs[:3]:
        first.step(*dev(b))
    sd = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in first.state_dict().items()}
    second, _, _, _ = fresh(shape, seed=10, table=table)      # other initial weights over the same frozen table: the rest comes from the state
    second.load_state_dict(sd)
    for b in bs[3:]:
        second.step(*dev(b))
    for name in ("params", "exp_avg", "exp_avg_sq", "step_count"):
        assert torch.equal(getattr(straight, name), getattr(second, name)), name
    assert int(second.step_count) == 6
    other, _, _, _ = fresh(HEADS[1])
    with pytest.raises(ValueError, match="another head"):
        other.load_state_dict(sd)


def test_the_model_reads_the_trained_buffer():
    from pmgt_amd.recommend import NcfScorer, host_scores, ncf_head_host, recommend
    shape = HEADS[0]
    tr, model, w, table = fresh(shape)
    table_d = tr.table
    for b in batches(4, 64):
        tr.step(*dev(b))
    sd = head_state(model)
    lo, hi = tr.params.data_ptr(), tr.params.data_ptr() + 4 * tr.params.numel()
    assert sorted(sd) == sorted(w) and all(lo <= t.data_ptr() < hi for t in sd.values())      # views, not copies
    now = {k: v.detach().cpu().numpy() for k, v in sd.items()}
    assert all(not np.array_equal(now[k], w[k]) for k in w)                                  # every tensor moved
    assert all(np.array_equal(now[k], tr.views(tr.params)[k].cpu().numpy()) for k in w)
    users = np.arange(USER_NUM)
    # model.head on the trained weights: against the fp64 formula on those weights
    o64 = ncf_head_host(now, users, table, np.float64)
    model.eval()
    s_h = host_scores(model, table_d, users)
    tol = 4 * max(np.abs(s_h - o64).max(), 2.0 ** -22 * np.abs(o64).max())
    assert np.abs(s_h - ncf_head_host(w, users, table, np.float64)).max() > 1e3 * tol           # not the initial weights
    s_d = NcfScorer(dict(sd), table_d).score(torch.from_numpy(users).cuda()).cpu().numpy()
    assert np.abs(s_d.astype(np.float64) - s_h).max() <= tol
    items, scores = recommend(model, None, users, k=5, table=table_d)
    assert np.abs(scores.astype(np.float64) - np.take_along_axis(s_h, items, axis=1)).max() <= tol
    # one more step is seen at once: nothing was copied
    tr.step(*dev(batches(1, 64, seed=8)[0]))
    assert np.abs(host_scores(model, table_d, users) - s_h).max() > 0


def test_refusals():
    model, w, table = make_model(16, 3, "MLP", USER_NUM, ITEM_NUM, 1)
    table_d = torch.from_numpy(table).cuda()
    for bad, what in ((table_d[:-1], "item table"), (table_d.double(), "item table"), (table_d.cpu(), "item table"), (table_d[:, :-8], "item table")):
        with pytest.raises(ValueError, match=what):
            NcfHeadTrainer(model, bad)
    model.emb_dropout.p = 0.1
    with pytest.raises(ValueError, match="dropout"):
        NcfHeadTrainer(model, table_d)
    model.emb_dropout.p = 0.0
    model.mlp_layers[1].dropout.p = 0.5
    with pytest.raises(ValueError, match="dropout"):
        NcfHeadTrainer(model, table_d)
    model.mlp_layers[1].dropout.p = 0.0
    model.factor_num = 12
    with pytest.raises(ValueError, match="factor_num"):
        NcfHeadTrainer(model, table_d)
    model.factor_num = 16
    tr = NcfHeadTrainer(model, table_d)
    with pytest.raises(RuntimeError, match="capture"):
        tr.replay()
    with pytest.raises(ValueError, match="int64"):
        tr.step(torch.zeros(4, dtype=torch.int32, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda"), torch.zeros(4, device="cuda"))
