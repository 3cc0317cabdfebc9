"""DcnTrainer.step: the gradient entry followed by ONE pmgt_op_adamw over the flat buffer -- bit-equal to the two calls made by hand, to its
own captured replay and across a state_dict round trip --, what decays and what never moves, and 20 steps against torch.

THE TRAJECTORY: 20 steps on batches of 33 pairs, lr 1e-3, weight_decay 0.01, clipping at 0.25 (it bites at every step: the norms are 0.33
to 1.2),
against pmgt_amd.dcn.DCN + autograd + clip_grad_norm_ + torch.optim.AdamW with the parameter groups the reference's get_optimizer forms
(decayed: every name without "bias"; tests/golden/dcn_grad.npz records that list) on the CPU in fp64 (o64) and in fp32 (r32), under the
project's measure on the 20 losses:  max|device - o64| <= 4 max(max|r32 - o64|, 2^-22 max|o64|).  Models (16, 1, 4, on) and (8, 2, 3, off).
On the CPU max|r32 - o64| is 9.4e-8 and 1.3e-7, below the floor of 2.0e-7 and 1.8e-7.  (At lr 1e-2 the LayerNorm model's fp32 torch
trajectory leaves the fp64 one by 0.08 within 20 steps: AdamW divides by the root of the second moment, so the DEGENERATE tensors, whose
gradient is rounding noise, take steps of size lr in directions that differ between any two realisations, and a 1 + s_c that such a step
carries across 0 flips the sign of LN(x0 (1 + s_c)).  The reference trains that way; a test of 20 steps at lr 1e-3 stays clear of it.)
Measured on the MI355X (one run): ratio 0.77 and 1.07."""
import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.dcn_head import decays
from pmgt_amd.dcn_train import DcnTrainer
from tests.dcn_util import C_BOUND, degenerate_keys, head_id, torch_model, world

pytestmark = pytest.mark.gpu

SETTINGS = dict(lr=1e-3, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8)
SHAPES = [(16, 1, 4, True), (8, 2, 3, False)]
BATCH, STEPS, CLIP = 33, 20, 0.25


def make(shape, clip=CLIP, **kw):
    h = world(shape)
    model = torch_model(h["w"], shape, device="cuda")
    trainer = DcnTrainer(model, max_grad_norm=clip, **{**SETTINGS, **kw})
    return h, model, trainer


def batches(h, steps=STEPS):
    rng = np.random.default_rng(7)
    for _ in range(steps):
        idx = rng.integers(0, len(h["users"]), size=BATCH)
        yield h["users"][idx], h["items"][idx], h["labels"][idx]


def dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


@pytest.mark.parametrize("clip", [CLIP, None], ids=["clip", "noclip"])
@pytest.mark.parametrize("shape", SHAPES, ids=head_id)
def test_a_step_is_the_gradient_entry_and_one_adamw_by_hand(shape, clip):
    h, model, trainer = make(shape, clip)
    _, _, other = make(shape, clip)
    lib = _lib.hip()
    scal, part = torch.zeros(8, device="cuda"), torch.zeros(1024, device="cuda")
    for users, items, labels in batches(h, 3):
        batch = dev(users, items, labels)
        loss = trainer.step(*batch).clone()
        loss2, _ = other.grad_fn(*batch)
        _lib.check(lib.pmgt_op_adamw(other.params.data_ptr(), other.grads.data_ptr(), other.exp_avg.data_ptr(), other.exp_avg_sq.data_ptr(),
                                     other.decay.data_ptr(), other.count, SETTINGS["lr"], SETTINGS["weight_decay"], 0.9, 0.999, 1e-8,
                                     float(clip or 0.0), other.step_count.data_ptr(), scal.data_ptr(), part.data_ptr(), _lib.stream()))
        assert torch.equal(loss, loss2) and torch.equal(trainer.params, other.params) and torch.equal(trainer.exp_avg_sq, other.exp_avg_sq)
    assert int(trainer.step_count[0]) == 3
    # the model's parameters are views of the buffer: its forward sees the trained weights
    users, items, labels = next(batches(h, 1))
    logits = trainer.grad_fn.forward(*dev(users, items))
    with torch.no_grad():
        assert torch.allclose(model(dev(users, items)), logits, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("shape", SHAPES, ids=head_id)
def test_replayed_steps_equal_eager_steps_and_a_state_round_trip_changes_nothing(shape):
    h, _, eager = make(shape)
    _, _, replayed = make(shape)
    _, _, resumed = make(shape)
    static = replayed.capture(BATCH)
    assert torch.equal(replayed.params, eager.params) and int(replayed.step_count[0]) == 0      # capturing left the state as it was
    losses = []
    for i, (users, items, labels) in enumerate(batches(h, 6)):
        batch = dev(users, items, labels)
        losses.append(eager.step(*batch).clone())
        if i < 3:
            for dst, src in zip(static[:3], batch):
                dst.copy_(src)
            assert torch.equal(replayed.replay(), losses[-1]) and torch.equal(replayed.params, eager.params)
        if i == 2:
            resumed.load_state_dict(replayed.state_dict())
        if i >= 3:
            assert torch.equal(resumed.step(*batch), losses[-1])
    assert torch.equal(resumed.params, eager.params) and torch.equal(resumed.exp_avg, eager.exp_avg) and int(resumed.step_count[0]) == 6
    _, _, other = make((8, 2, 3, True) if shape[3] is False else (16, 1, 4, False))
    with pytest.raises(ValueError, match="layouts differ"):
        other.load_state_dict(eager.state_dict())
    with pytest.raises(RuntimeError, match="capture"):
        eager.replay()


def test_what_decays_and_what_never_moves():
    shape = (16, 1, 4, True)
    h, model, trainer = make(shape, clip=None, weight_decay=0.1)
    views = trainer.views(trainer.params)
    dmask = trainer.views(trainer.decay)
    for k in views:
        assert bool(dmask[k].all()) == decays(k) and bool(dmask[k].any()) == decays(k), k
    cross_bias = {c: getattr(model.cross_net.layers, str(c)).bias for c in range(shape[2])}
    assert all(b.data_ptr() < trainer.params.data_ptr() or b.data_ptr() >= trainer.params.data_ptr() + 4 * trainer.count for b in cross_bias.values())
    before_bias = {c: b.detach().clone() for c, b in cross_bias.items()}
    before = {k: v.detach().clone() for k, v in views.items()}
    for users, items, labels in batches(h, 20):
        trainer.step(*dev(users, items, labels))
    torch.cuda.synchronize()
    for c, b in cross_bias.items():                          # never read, no gradient, never stepped: the same bits
        assert torch.equal(b.detach().view(torch.int32), before_bias[c].view(torch.int32)) and b.grad is None, c
    assert "cross_net.layers.0.bias" in model.state_dict() and "cross_net.layers.0.bias" not in trainer.layout
    # everything else moved, but for the degenerate tensors without decay: the gradient of an inner cross layer's beta is rounding noise
    # of rounding noise (1e-14 and below), far under AdamW's eps, so its step vanishes next to a beta of size 0.3
    still_ok = [k for k in degenerate_keys(shape) if not decays(k)]
    assert all(not torch.equal(views[k], before[k]) for k in views if k not in still_ok)
    # a zero gradient: layer_norm.weight still moves, by the decay alone; layer_norm.bias does not move at all
    _, _, still = make(shape, clip=None, weight_decay=0.1)
    g0 = still.views(still.params)
    b0 = {k: v.detach().clone() for k, v in g0.items()}
    still.grads.zero_()
    _lib.check(_lib.hip().pmgt_op_adamw(still.params.data_ptr(), still.grads.data_ptr(), still.exp_avg.data_ptr(), still.exp_avg_sq.data_ptr(),
                                        still.decay.data_ptr(), still.count, 1e-2, 0.1, 0.9, 0.999, 1e-8, 0.0, still.step_count.data_ptr(),
                                        still._scal.data_ptr(), still._part.data_ptr(), _lib.stream()))
    for k in g0:
        if k.endswith("layer_norm.weight"):
            assert torch.allclose(g0[k], b0[k] * (1 - 1e-2 * 0.1), rtol=1e-6, atol=0) and not torch.equal(g0[k], b0[k]), k
        if k.endswith("bias"):
            assert torch.equal(g0[k], b0[k]), k


def torch_trajectory(h, shape, dtype):
    model = torch_model(h["w"], shape, dtype)
    named = [(k, p) for k, p in model.named_parameters()]
    recorded = np.load(__file__.replace("test_dcn_step_gpu.py", "golden/dcn_grad.npz"))
    tag = "run" if shape == (16, 1, 4, True) else "noln"
    decayed = set(str(k) for k in recorded[tag + "/decayed"])
    assert decayed == {k for k, _ in named if "bias" not in k}
    opt = torch.optim.AdamW([{"params": [p for k, p in named if k in decayed], "weight_decay": SETTINGS["weight_decay"]},
                             {"params": [p for k, p in named if k not in decayed], "weight_decay": 0.0}],
                            lr=SETTINGS["lr"], betas=SETTINGS["betas"], eps=SETTINGS["eps"])
    losses, norms = [], []
    for users, items, labels in batches(h):
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(model((torch.from_numpy(users), torch.from_numpy(items))),
                                                                    torch.from_numpy(labels).to(dtype))
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_([p for _, p in named if p.grad is not None], CLIP)))
        opt.step()
        losses.append(float(loss.item()))
    return np.asarray(losses), norms


@pytest.mark.parametrize("shape", SHAPES, ids=head_id)
def test_twenty_steps_follow_torch(shape):
    h, _, trainer = make(shape)
    o64, norms = torch_trajectory(h, shape, torch.float64)
    r32, _ = torch_trajectory(h, shape, torch.float32)
    assert min(norms) > CLIP                             # the clipping bites
    losses = torch.empty(STEPS, 1, device="cuda")
    for s, (users, items, labels) in enumerate(batches(h)):
        trainer.step(*dev(users, items, labels), loss=losses[s])
    got = losses.cpu().numpy().reshape(-1).astype(np.float64)
    scale = max(np.abs(r32 - o64).max(), 2.0 ** -22 * np.abs(o64).max())
    ratio = np.abs(got - o64).max() / scale
    print(f"{head_id(shape)}: loss {o64[0]:.4f} -> {o64[-1]:.4f}, max|device - o64| {np.abs(got - o64).max():.3g}, "
          f"max|r32 - o64| {np.abs(r32 - o64).max():.3g}, ratio {ratio:.2f}")
    assert np.isfinite(got).all() and ratio <= C_BOUND
