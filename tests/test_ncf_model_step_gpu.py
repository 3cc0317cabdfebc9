"""NcfModelTrainer.step: the gradient entry followed by ONE pmgt_op_adamw over the flat buffer -- bit-equal to the two calls made by hand,
to its own captured replay and across a state_dict round trip --, what decays, what stays outside the buffer and never moves, and 20 steps
against torch.

THE TRAJECTORY: 20 steps on batches of 33 pairs, lr 1e-3, weight_decay 0.01, clipping at 0.25, against pmgt_amd.ncf.NCF + autograd +
clip_grad_norm_ + torch.optim.AdamW with the parameter groups the reference's get_optimizer forms (decayed: every name without "bias" or
"LayerNorm.weight"; tests/golden/ncf_model.npz records that list) on the CPU in fp64 (o64) and in fp32 (r32), under the project's measure on
the 20 losses:  max|device - o64| <= 4 max(max|r32 - o64|, 2^-22 max|o64|).  Models (8, 2, NeuMF-end, LayerNorm on) and (8, 2, GMF).
On the CPU max|r32 - o64| is 1.3e-7 and 2.1e-7 (3.1e-7 for the second model in the run on the MI355X host), at or below the floors of 2.0e-7 and 2.3e-7; the gradient
norms are 0.28 to 0.84, so the clipping bites at every step.  Measured on the MI355X (one run): ratio 0.72 and 0.84."""
import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.ncf_model import ITEM_MLP
from pmgt_amd.ncf_model_train import NcfModelTrainer, decays
from tests.dcn_util import C_BOUND
from tests.ncf_model_util import GOLD, head_id, torch_model, world

pytestmark = pytest.mark.gpu

SETTINGS = dict(lr=1e-3, weight_decay=0.01, betas=(0.9, 0.999), eps=1e-8)
SHAPES = [(8, 2, "NeuMF-end", True), (8, 2, "GMF", False)]
TAG = {SHAPES[0]: "neumf_ln", SHAPES[1]: "gmf"}
BATCH, STEPS, CLIP = 33, 20, 0.25


def make(shape, clip=CLIP, **kw):
    h = world(shape)
    model = torch_model(h["w"], shape, device="cuda")
    trainer = NcfModelTrainer(model, max_grad_norm=clip, **{**SETTINGS, **kw})
    return h, model, trainer


def batches(h, steps=STEPS):
    rng = np.random.default_rng(7)
    for _ in range(steps):
        idx = rng.integers(0, len(h["users"]), size=BATCH)
        yield h["users"][idx], h["items"][idx], h["labels"][idx]


def dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


@pytest.mark.parametrize("clip", [CLIP, None], ids=["clip", "noclip"])
@pytest.mark.parametrize("shape", SHAPES + [(16, 3, "MLP", False)], ids=head_id)
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
    # the model's parameters are views of the buffer: its forward sees the trained weights, and trainer.table is embed_item_MLP
    users, items, labels = next(batches(h, 1))
    _, logits = trainer.grad_fn(*dev(users, items, labels))
    with torch.no_grad():
        assert torch.allclose(model.eval()(dev(users, items)), logits, rtol=1e-4, atol=1e-5)
    if shape[2] != "GMF":
        assert trainer.table.data_ptr() == model.embed_item_MLP.weight.data_ptr() == trainer.params.data_ptr() + 4 * trainer.layout[ITEM_MLP][0]


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
    _, _, other = make(shape, freeze_items=True) if shape[2] != "GMF" else make(SHAPES[0])
    with pytest.raises(ValueError, match="layouts differ"):
        other.load_state_dict(eager.state_dict())
    with pytest.raises(RuntimeError, match="capture"):
        eager.replay()


@pytest.mark.parametrize("shape", SHAPES, ids=head_id)
def test_the_decay_mask_is_the_reference_optimizers_decayed_group(shape):
    _, model, trainer = make(shape, clip=None)
    decayed = set(str(k) for k in GOLD[TAG[shape] + "/decayed"])
    dmask = trainer.views(trainer.decay)
    for k in dmask:
        assert bool(dmask[k].all()) == bool(dmask[k].any()) == (k in decayed) == decays(k), k
    assert set(dmask) == {k for k, _ in model.named_parameters()} - set(str(k) for k in GOLD[TAG[shape] + "/nograd"])
    if shape[3]:
        assert dmask["MLP_layers.2.weight"].all() and not dmask["MLP_layers.2.bias"].any()      # the gammas decay, the betas do not


def outside(trainer, p):
    return p.data_ptr() < trainer.params.data_ptr() or p.data_ptr() >= trainer.params.data_ptr() + 4 * trainer.count


@pytest.mark.parametrize("kind", ("MLP", "GMF", "NeuMF-pre", "frozen"))
def test_tensors_outside_the_buffer_keep_their_bits(kind):
    shape = (8, 2, "NeuMF-end" if kind == "frozen" else kind, True)
    h = world(shape if kind != "NeuMF-pre" else (8, 2, "NeuMF-end", True))
    kwargs = {}
    if kind == "NeuMF-pre":
        gmf = torch_model(world((8, 2, "GMF", False))["w"], (8, 2, "GMF", False))
        mlp = torch_model(world((8, 2, "MLP", True))["w"], (8, 2, "MLP", True))
        kwargs = dict(GMF_model=gmf, MLP_model=mlp, alpha=0.3)
    model = torch_model({} if kind == "NeuMF-pre" else h["w"], shape, device="cuda", user_num=5, item_num=7, **kwargs)
    trainer = NcfModelTrainer(model, max_grad_norm=CLIP, freeze_items=kind == "frozen", **SETTINGS)
    named = dict(model.named_parameters())
    out = {k: p for k, p in named.items() if k not in trainer.layout}
    expect = {"MLP": {"embed_user_GMF.weight", "embed_item_GMF.weight"},
              "GMF": {"embed_user_MLP.weight", "embed_item_MLP.weight"} | {k for k in named if k.startswith("MLP_layers.")},
              "NeuMF-pre": {k for k in named if k.startswith(("GMF_model.", "MLP_model."))}, "frozen": {"embed_item_MLP.weight"}}[kind]
    assert set(out) == expect and all(outside(trainer, p) for p in out.values())
    assert all(not outside(trainer, named[k]) for k in trainer.layout)
    before = {k: p.detach().clone() for k, p in out.items()}
    inside = trainer.params.clone()
    table = trainer.table.clone()
    for users, items, labels in batches(h, 5):
        trainer.step(*dev(users, items, labels))
    torch.cuda.synchronize()
    for k, p in out.items():
        assert torch.equal(p.detach().view(torch.int32), before[k].view(torch.int32)) and p.grad is None, k
    views, then = trainer.views(trainer.params), trainer.views(inside)
    assert all(not torch.equal(views[k], then[k]) for k in views)
    if kind == "frozen":
        assert outside(trainer, trainer.table) and torch.equal(trainer.table, table) and trainer.table.data_ptr() != named[ITEM_MLP].data_ptr()
    assert set(model.state_dict()) >= set(trainer.layout) | set(out)


def test_a_model_with_dropout_needs_a_seed_and_then_trains_with_fresh_masks():
    shape = SHAPES[0]
    h = world(shape)
    model = torch_model(h["w"], shape, device="cuda", emb_dropout=0.2, dropout=0.2)
    with pytest.raises(ValueError, match="dropout_seed"):
        NcfModelTrainer(model)
    gmf = torch_model(world(SHAPES[1])["w"], SHAPES[1], device="cuda", dropout=0.5)      # kind GMF reads no layer: its layers' p do not count
    NcfModelTrainer(gmf)
    a = NcfModelTrainer(model, dropout_seed=11, **SETTINGS)
    b = NcfModelTrainer(torch_model(h["w"], shape, device="cuda", emb_dropout=0.2, dropout=0.2), dropout_seed=11, **SETTINGS)
    batch = dev(*next(batches(h, 1)))
    l0, l1 = a.step(*batch).clone(), a.step(*batch).clone()
    static = b.capture(BATCH)
    for dst, src in zip(static[:3], batch):
        dst.copy_(src)
    assert torch.equal(b.replay().clone(), l0) and torch.equal(b.replay().clone(), l1) and torch.equal(a.params, b.params)
    assert int(a.rng[1]) == 2 and not torch.equal(l0, l1)


def torch_trajectory(h, shape, dtype):
    model = torch_model(h["w"], shape, dtype).eval()
    named = [(k, p) for k, p in model.named_parameters()]
    decayed = set(str(k) for k in GOLD[TAG[shape] + "/decayed"])
    assert decayed == {k for k, _ in named if decays(k)}
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
    assert min(norms) > CLIP                             # the clipping bites at every step (norms 0.28 to 0.78)
    losses = torch.empty(STEPS, 1, device="cuda")
    for s, (users, items, labels) in enumerate(batches(h)):
        trainer.step(*dev(users, items, labels), loss=losses[s])
    got = losses.cpu().numpy().reshape(-1).astype(np.float64)
    scale = max(np.abs(r32 - o64).max(), 2.0 ** -22 * np.abs(o64).max())
    ratio = np.abs(got - o64).max() / scale
    print(f"{head_id(shape)}: loss {o64[0]:.4f} -> {o64[-1]:.4f}, max|device - o64| {np.abs(got - o64).max():.3g}, "
          f"max|r32 - o64| {np.abs(r32 - o64).max():.3g}, ratio {ratio:.2f}")
    assert np.isfinite(got).all() and ratio <= C_BOUND
