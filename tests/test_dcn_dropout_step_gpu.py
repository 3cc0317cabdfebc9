"""DcnTrainer(dropout_seed=...).step: pmgt_dcn_train_grad_dropout followed by ONE pmgt_op_adamw over the flat buffer, whose step counter IS
the step of the mask stream -- bit-equal to the two calls made by hand, to its own captured replay and across a state_dict round trip;
fresh masks at every replay with no host write; a pure function of the seed -- and 20 steps against torch UNDER THE HOST MASKS.

THE TRAJECTORY: tests/test_dcn_step_gpu.py's two models, batches and settings (20 steps on batches of 33 pairs, lr 1e-3, weight_decay
0.01, clipping at 0.25) with emb_dropout 0.2 and dropout 0.3 (deep and cross), against pmgt_amd.dcn.DCN + autograd + clip_grad_norm_ +
torch.optim.AdamW on the CPU in fp64 (o64) and in fp32 (r32), the model's Dropout modules replaced at step s by the stubs of
dcn_dropout_masks(seed, s, ...): the masks the device draws when its step counter reads s.  The project's measure on the 20 losses:
    max|device - o64| <= 4 max(max|r32 - o64|, 2^-22 max|o64|)."""
import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.dcn_head import dcn_dropout_masks
from pmgt_amd.dcn_train import DcnGrad, DcnTrainer
from tests.dcn_dropout_util import set_dropout, set_stubs
from tests.dcn_util import C_BOUND, EPS, head_id, torch_model, world
from tests.test_dcn_step_gpu import BATCH, CLIP, SETTINGS, SHAPES, STEPS, batches, dev

pytestmark = pytest.mark.gpu

SEED = -0x1234_5678_9ABC                                     # (negative: the int64 pair holds it as it is)
P_EMB, P = 0.2, 0.3


def make(shape, seed=SEED, clip=CLIP, **kw):
    h = world(shape)
    model = set_dropout(torch_model(h["w"], shape, device="cuda"), P_EMB, P)
    trainer = DcnTrainer(model, max_grad_norm=clip, dropout_seed=seed, **{**SETTINGS, **kw})
    return h, model, trainer


@pytest.mark.parametrize("shape", SHAPES, ids=head_id)
def test_a_step_is_the_dropout_entry_and_one_adamw_by_hand(shape):
    h, model, trainer = make(shape)
    _, other_model, other = make(shape)
    other_model.train()                                      # the step is a training step whatever model.training says
    assert not model.training and trainer.rng.tolist() == [SEED, 0] and trainer.step_count.data_ptr() == trainer.rng.data_ptr() + 8
    lib = _lib.hip()
    scal, part = torch.zeros(8, device="cuda"), torch.zeros(1024, device="cuda")
    plain = DcnGrad(*shape, EPS, model.user_num, model.item_num, other.params, torch.zeros_like(other.grads))      # the entry without dropout
    for users, items, labels in batches(h, 3):
        batch = dev(users, items, labels)
        undropped, _ = plain(*batch)
        loss = trainer.step(*batch).clone()
        loss2, _ = other.grad_fn(*batch)
        _lib.check(lib.pmgt_op_adamw(other.params.data_ptr(), other.grads.data_ptr(), other.exp_avg.data_ptr(), other.exp_avg_sq.data_ptr(),
                                     other.decay.data_ptr(), other.count, SETTINGS["lr"], SETTINGS["weight_decay"], 0.9, 0.999, 1e-8,
                                     float(CLIP), other.rng[1:2].data_ptr(), scal.data_ptr(), part.data_ptr(), _lib.stream()))
        assert torch.equal(loss, loss2) and torch.equal(trainer.params, other.params) and torch.equal(trainer.exp_avg_sq, other.exp_avg_sq)
        assert not torch.equal(loss, undropped)              # (it is the training-mode loss)
    assert int(trainer.step_count[0]) == 3 and trainer.rng.tolist() == [SEED, 3]
    # the forward entry and the model's own eval forward never drop
    users, items, labels = next(batches(h, 1))
    logits = trainer.grad_fn.forward(*dev(users, items))
    assert torch.equal(logits, DcnGrad(*shape, EPS, model.user_num, model.item_num, trainer.params).forward(*dev(users, items)))
    with torch.no_grad():
        assert torch.allclose(model(dev(users, items)), logits, rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("shape", SHAPES, ids=head_id)
def test_replayed_steps_equal_eager_steps_and_a_state_round_trip_changes_nothing(shape):
    h, _, eager = make(shape)
    _, _, replayed = make(shape)
    _, _, resumed = make(shape)
    static = replayed.capture(BATCH)
    assert torch.equal(replayed.params, eager.params) and replayed.rng.tolist() == [SEED, 0]      # capturing left the state as it was
    losses = []
    for i, (users, items, labels) in enumerate(batches(h, 6)):
        batch = dev(users, items, labels)
        losses.append(eager.step(*batch).clone())
        if i < 3:
            for dst, src in zip(static[:3], batch):
                dst.copy_(src)
            assert torch.equal(replayed.replay(), losses[-1]) and torch.equal(replayed.params, eager.params)
        if i == 2:
            sd = replayed.state_dict()
            assert sd["dropout_seed"] == SEED and int(sd["step"][0]) == 3
            resumed.load_state_dict(sd)
        if i >= 3:
            assert torch.equal(resumed.step(*batch), losses[-1])
    assert torch.equal(resumed.params, eager.params) and torch.equal(resumed.exp_avg, eager.exp_avg) and resumed.rng.tolist() == [SEED, 6]
    _, _, other_seed = make(shape, seed=SEED + 1)
    with pytest.raises(ValueError, match="dropout_seed"):
        other_seed.load_state_dict(eager.state_dict())
    unseeded = DcnTrainer(torch_model(h["w"], shape, device="cuda"), max_grad_norm=CLIP, **SETTINGS)
    with pytest.raises(ValueError, match="dropout_seed"):
        unseeded.load_state_dict(eager.state_dict())
    with pytest.raises(ValueError, match="dropout_seed"):
        eager.load_state_dict(unseeded.state_dict())


def test_replays_draw_fresh_masks_and_another_seed_gives_other_parameters():
    shape = SHAPES[0]
    h, _, trainer = make(shape, lr=0.0, weight_decay=0.0)
    static = trainer.capture(BATCH)
    for dst, src in zip(static[:3], dev(*next(batches(h, 1)))):
        dst.copy_(src)
    before = trainer.params.clone()
    fresh = [float(trainer.replay()[0]) for _ in range(3)]   # lr 0: one batch, the same parameters, the step counter 0, 1, 2
    assert len(set(fresh)) == 3 and torch.equal(trainer.params, before) and int(trainer.step_count[0]) == 3
    same = []
    for _ in range(3):
        trainer.rng[1] = 0
        same.append(float(trainer.replay()[0]))
    assert len(set(same)) == 1 and same[0] == fresh[0]
    _, _, a = make(shape)
    _, _, b = make(shape, seed=SEED + 1)
    _, _, c = make(shape)
    for users, items, labels in batches(h, 2):
        for t in (a, b, c):
            t.step(*dev(users, items, labels))
    assert torch.equal(a.params, c.params) and not torch.equal(a.params, b.params)


def test_a_model_with_dropout_and_no_seed_is_refused_and_so_is_a_bad_seed_or_p():
    shape = SHAPES[0]
    h = world(shape)
    model = set_dropout(torch_model(h["w"], shape, device="cuda"), P_EMB, P)
    with pytest.raises(ValueError, match="dropout is not covered"):
        DcnTrainer(model)
    for seed in (True, 1.5, 2 ** 63):
        with pytest.raises(ValueError, match="dropout_seed"):
            DcnTrainer(model, dropout_seed=seed)
    model.cross_net.layers[1].dropout.p = 1.0
    with pytest.raises(ValueError, match="cross layer 1"):
        DcnTrainer(model, dropout_seed=3)


def torch_trajectory(h, shape, dtype):
    model = set_dropout(torch_model(h["w"], shape, dtype), P_EMB, P)
    named = [(k, p) for k, p in model.named_parameters()]
    opt = torch.optim.AdamW([{"params": [p for k, p in named if "bias" not in k], "weight_decay": SETTINGS["weight_decay"]},
                             {"params": [p for k, p in named if "bias" in k], "weight_decay": 0.0}],
                            lr=SETTINGS["lr"], betas=SETTINGS["betas"], eps=SETTINGS["eps"])
    losses, norms = [], []
    for s, (users, items, labels) in enumerate(batches(h)):
        set_stubs(model, dcn_dropout_masks(SEED, s, BATCH, *shape[:3], P_EMB, P, P), dtype)
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(model((torch.from_numpy(users), torch.from_numpy(items))),
                                                                    torch.from_numpy(labels).to(dtype))
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_([p for _, p in named if p.grad is not None], CLIP)))
        opt.step()
        losses.append(float(loss.item()))
    return np.asarray(losses), norms


@pytest.mark.parametrize("shape", SHAPES, ids=head_id)
def test_twenty_steps_follow_torch_under_the_host_masks(shape):
    h, _, trainer = make(shape)
    o64, norms = torch_trajectory(h, shape, torch.float64)
    r32, _ = torch_trajectory(h, shape, torch.float32)
    assert min(norms) > CLIP                                 # the clipping bites
    losses = torch.empty(STEPS, 1, device="cuda")
    for s, (users, items, labels) in enumerate(batches(h)):
        trainer.step(*dev(users, items, labels), loss=losses[s])
    got = losses.cpu().numpy().reshape(-1).astype(np.float64)
    scale = max(np.abs(r32 - o64).max(), 2.0 ** -22 * np.abs(o64).max())
    ratio = np.abs(got - o64).max() / scale
    print(f"{head_id(shape)}: loss {o64[0]:.4f} -> {o64[-1]:.4f}, max|device - o64| {np.abs(got - o64).max():.3g}, "
          f"max|r32 - o64| {np.abs(r32 - o64).max():.3g}, ratio {ratio:.2f}")
    assert np.isfinite(got).all() and ratio <= C_BOUND


if __name__ == "__main__":                                   # the CPU side of the trajectory: no GPU is needed
    for shape in SHAPES:
        h = world(shape)
        o64, norms = torch_trajectory(h, shape, torch.float64)
        r32, _ = torch_trajectory(h, shape, torch.float32)
        print(head_id(shape), f"loss {o64[0]:.4f} -> {o64[-1]:.4f}, norms {min(norms):.2f} .. {max(norms):.2f}, max|r32 - o64| "
              f"{np.abs(r32 - o64).max():.3g}, floor {2.0 ** -22 * np.abs(o64).max():.3g}")
