"""PairTrainer's options -- optim, the learning-rate schedule, the step guard -- on the three pair trainers, each at the smallest head its own
step test covers: NcfHeadTrainer (16, 3, NeuMF-end) of tests/test_ncf_train_step_gpu.py, DcnTrainer (8, 2, 3, no LayerNorm) of
tests/test_dcn_step_gpu.py, NcfModelTrainer (8, 2, NeuMF-end, LayerNorm) of tests/test_ncf_model_step_gpu.py.

  * A default-keyword trainer's step is the gradient entry plus one pmgt_op_adamw by hand, bit for bit: the path from before the options.
  * Twenty steps follow torch (SGD under `linear` with warm-up; AdamW under `cosine`) by the measure of test_twenty_steps_follow_torch in
    tests/test_dcn_step_gpu.py: max|device - fp64 torch| <= C_BOUND max(max|fp32 torch - fp64 torch|, 2^-22 max|fp64 torch|), C_BOUND imported.
  * The guard, with every id in range: ONE user's embedding row is Inf.  A batch with that user is skipped (parameters, moments, step
    bit-identical), batches without apply, check_nonfinite raises after max_skipped_in_a_row, the log ring tells what was done.
  * Replayed steps equal eager steps, a skipped one among them; the state round trip; the refusals; no moments under SGD."""
import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.dcn_head import USER_KEY
from pmgt_amd.dcn_head import decays as dcn_decays
from pmgt_amd.dcn_train import DcnTrainer
from pmgt_amd.ncf_model import USER_GMF, USER_MLP
from pmgt_amd.ncf_model_train import NcfModelTrainer
from pmgt_amd.ncf_model_train import decays as ncf_model_decays
from pmgt_amd.ncf_train import NcfHeadTrainer
from pmgt_amd.schedule import lr_lambda
from pmgt_amd.trainer import NonFiniteGradientsError
from tests import dcn_util, ncf_model_util
from tests.dcn_util import C_BOUND
from tests.ncf_train_util import TorchHead, make_model
from tests.test_recommend_cpu import random_head

pytestmark = pytest.mark.gpu

KINDS = ["ncf_head", "dcn", "ncf_model"]
STEPS, WARMUP, BATCH, WD = 20, 3, 33, 0.01
DCN_SHAPE, NCF_MODEL_SHAPE, NCF_HEAD = (8, 2, 3, False), (8, 2, "NeuMF-end", True), (16, 3, "NeuMF-end")
HEAD_USERS, HEAD_ITEMS = 23, 41
LR = {"adamw": 1e-3, "sgd": 0.05}
CLIP = {"ncf_head": 5.0, "dcn": 0.25, "ncf_model": 0.25}      # the step tests' own


def world_of(kind):
    """the weights and a pair list whose LAST user never appears"""
    if kind == "dcn":
        return dcn_util.world(DCN_SHAPE)
    if kind == "ncf_model":
        return ncf_model_util.world(NCF_MODEL_SHAPE)
    rng = np.random.default_rng(3)
    n = 130
    return dict(users=rng.integers(0, HEAD_USERS - 1, size=n), items=rng.integers(0, HEAD_ITEMS, size=n),
                labels=(rng.random(n) < 0.4).astype(np.float32), user_num=HEAD_USERS)


def make(kind, optim="adamw", **kw):
    """(trainer, the names of the user tables in its layout)"""
    h = world_of(kind)
    hyper = dict(lr=LR.get(optim, 1e-3), weight_decay=WD, max_grad_norm=CLIP[kind], optim=optim, **kw)
    if kind == "dcn":
        return DcnTrainer(dcn_util.torch_model(h["w"], DCN_SHAPE, device="cuda"), **hyper), [USER_KEY]
    if kind == "ncf_model":
        return NcfModelTrainer(ncf_model_util.torch_model(h["w"], NCF_MODEL_SHAPE, device="cuda"), **hyper), [USER_MLP, USER_GMF]
    model, _, table = make_model(*NCF_HEAD, HEAD_USERS, HEAD_ITEMS, 9)      # (random_head(..., 9)'s weights and table)
    return NcfHeadTrainer(model, torch.from_numpy(table).cuda(), **hyper), ["mlp_user_embeddings.weight", "gmf_user_embeddings.weight"]


def batches(kind, steps=STEPS):
    h = world_of(kind)
    rng = np.random.default_rng(7)
    out = []
    for _ in range(steps):
        idx = rng.integers(0, len(h["users"]), size=BATCH)
        out.append((h["users"][idx], h["items"][idx], h["labels"][idx]))
    return out


def dev(batch):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in batch)


def with_user(batch, user):
    users = batch[0].copy()
    users[len(users) // 2] = user
    return users, batch[1], batch[2]


def bits(t):
    return t.detach().view(torch.int32)


def same_state(a, b):
    """two trainers, or a trainer and a state_dict of clones: parameters, moments and step bit for bit"""
    b = b if isinstance(b, dict) else b.state_dict()
    sd = a.state_dict()
    assert set(sd) == set(b)
    return all(torch.equal(bits(sd[k]), bits(b[k])) if k != "step" else torch.equal(sd[k], b[k])
               for k in ("params", "exp_avg", "exp_avg_sq", "step") if k in sd)


# ---- the default path -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_a_default_trainer_steps_through_pmgt_op_adamw_as_ever(kind):
    trainer, _ = make(kind)
    other, _ = make(kind)
    assert trainer._guard_state is None and trainer._sched is None and trainer._scal.numel() == 8 and trainer._part.numel() == 1024
    scal, part = torch.zeros(8, device="cuda"), torch.zeros(1024, device="cuda")
    for batch in batches(kind, 3):
        b = dev(batch)
        loss = trainer.step(*b).clone()
        loss2, _ = other.grad_fn(*b)
        _lib.check(_lib.hip().pmgt_op_adamw(other.params.data_ptr(), other.grads.data_ptr(), other.exp_avg.data_ptr(), other.exp_avg_sq.data_ptr(),
                                            other.decay.data_ptr(), other.count, LR["adamw"], WD, 0.9, 0.999, 1e-8, CLIP[kind],
                                            other.step_count.data_ptr(), scal.data_ptr(), part.data_ptr(), _lib.stream()))
        assert torch.equal(loss, loss2) and same_state(trainer, other)
    assert int(trainer.step_count[0]) == 3 and trainer.step_log() == [] and trainer.check_nonfinite() is None
    sd = trainer.state_dict()
    assert sd["optim"] == "adamw" and sd["schedule"] is None and "step_counters" not in sd and "step_log" not in sd


# ---- twenty steps against torch ------------------------------------------------------------------------------------------------------------
def torch_losses(kind, optim, sched, dtype):
    h = world_of(kind)
    if kind == "ncf_head":
        w, table = random_head(*NCF_HEAD, HEAD_USERS, HEAD_ITEMS, 9)
        head = TorchHead(w, table, dtype, lr=LR[optim])
        named, decays = list(head.p.items()), lambda k: not k.endswith(".bias")
        forward = head.logits
    else:
        model = (dcn_util.torch_model(h["w"], DCN_SHAPE, dtype) if kind == "dcn" else ncf_model_util.torch_model(h["w"], NCF_MODEL_SHAPE, dtype)).eval()
        named, decays = list(model.named_parameters()), dcn_decays if kind == "dcn" else ncf_model_decays
        forward = lambda users, items: model((torch.from_numpy(users), torch.from_numpy(items)))
    groups = [{"params": [p for k, p in named if decays(k)], "weight_decay": WD}, {"params": [p for k, p in named if not decays(k)], "weight_decay": 0.0}]
    opt = torch.optim.SGD(groups, lr=LR[optim]) if optim == "sgd" else torch.optim.AdamW(groups, lr=LR[optim], betas=(0.9, 0.999), eps=1e-8)
    lr_sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda(sched, WARMUP, STEPS, LR[optim]))
    losses, norms = [], []
    for users, items, labels in batches(kind):
        opt.zero_grad(set_to_none=True)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(forward(users, items), torch.from_numpy(labels).to(dtype))
        loss.backward()
        norms.append(float(torch.nn.utils.clip_grad_norm_([p for _, p in named if p.grad is not None], CLIP[kind])))
        opt.step()
        lr_sched.step()
        losses.append(float(loss.item()))
    return np.asarray(losses), norms


@pytest.mark.parametrize("optim,sched", [("sgd", "linear"), ("adamw", "cosine")])
@pytest.mark.parametrize("kind", KINDS)
def test_twenty_scheduled_steps_follow_torch(kind, optim, sched):
    """Measured on the MI355X (one run; the ratio of the assertion, against C_BOUND = 4), NcfHeadTrainer / DcnTrainer / NcfModelTrainer:
    SGD under `linear` 0.76 / 0.62 / 0.93, AdamW under `cosine` 0.70 / 1.00 / 0.71."""
    trainer, _ = make(kind, optim, scheduler_type=sched, num_warmup_steps=WARMUP, num_training_steps=STEPS)
    o64, norms = torch_losses(kind, optim, sched, torch.float64)
    r32, _ = torch_losses(kind, optim, sched, torch.float32)
    losses = torch.empty(STEPS, 1, device="cuda")
    for s, batch in enumerate(batches(kind)):
        trainer.step(*dev(batch), loss=losses[s])
    got = losses.cpu().numpy().reshape(-1).astype(np.float64)
    scale = max(np.abs(r32 - o64).max(), 2.0 ** -22 * np.abs(o64).max())
    ratio = np.abs(got - o64).max() / scale
    print(f"{kind} {optim} {sched}: loss {o64[0]:.4f} -> {o64[-1]:.4f}, grad norms {min(norms):.3g} .. {max(norms):.3g}, "
          f"max|device - o64| {np.abs(got - o64).max():.3g}, max|r32 - o64| {np.abs(r32 - o64).max():.3g}, ratio {ratio:.2f}")
    assert int(trainer.step_count[0]) == STEPS
    assert not np.array_equal(o64[1:], o64[:-1]) and np.isfinite(got).all() and ratio <= C_BOUND


# ---- the guard --------------------------------------------------------------------------------------------------------------------------------
def poison(trainer, user_keys, user):
    with torch.no_grad():
        for k in user_keys:
            trainer.views(trainer.params)[k][user] = float("inf")


@pytest.mark.parametrize("optim", ["adamw", "sgd"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_batch_with_the_inf_user_is_skipped_and_the_others_apply(kind, optim):
    bad_user = world_of(kind)["user_num"] - 1
    trainer, user_keys = make(kind, optim, scheduler_type="linear", num_warmup_steps=0, num_training_steps=STEPS, nonfinite="skip", step_log=8,
                              max_skipped_in_a_row=3)                                       # (no warm-up: the first step's rate is not 0)
    assert (trainer.exp_avg is None) == (optim == "sgd")
    poison(trainer, user_keys, bad_user)
    bs = batches(kind, 6)
    plan = [False, True, False, True, True, True]            # which steps carry the Inf user
    losses, applied = [], 0
    for batch, bad in zip(bs, plan):
        before = trainer.state_dict()
        losses.append(float(trainer.step(*dev(with_user(batch, bad_user) if bad else batch))))
        if bad:
            assert same_state(trainer, before)               # parameters, moments and step: bit-identical
            c = trainer.step_counters()
        else:
            applied += 1
            assert not torch.equal(bits(trainer.params), bits(before["params"])) and trainer.check_nonfinite()["skipped_in_a_row"] == 0
        assert int(trainer.step_count[0]) == applied
    assert c == {"attempts": 6, "skipped": 4, "skipped_in_a_row": 3}
    with pytest.raises(NonFiniteGradientsError, match="3 optimizer steps in a row"):
        trainer.check_nonfinite()
    log = trainer.step_log()
    assert [r["attempt"] for r in log] == list(range(6)) and [r["skipped"] for r in log] == plan == [r["nonfinite"] for r in log]
    assert [r["opt_step"] for r in log] == [1, 1, 2, 2, 2, 2]
    lam = lr_lambda("linear", 0, STEPS, LR[optim])
    for r, loss, bad in zip(log, losses, plan):
        assert (np.isnan(r["loss"]) and np.isnan(loss)) or r["loss"] == loss               # the step's own loss
        assert np.isfinite(r["grad_norm"]) != bad and (r["clip_coef"] == 0.0) == bad
        done = r["opt_step"] - (0 if bad else 1)                                            # the steps completed before this one
        assert r["lr"] == pytest.approx(LR[optim] * lam(done), rel=1e-6, abs=0)


@pytest.mark.parametrize("optim", ["adamw", "sgd"])
@pytest.mark.parametrize("kind", KINDS)
def test_replayed_steps_equal_eager_steps_a_skipped_one_among_them(kind, optim):
    bad_user = world_of(kind)["user_num"] - 1
    opts = dict(scheduler_type="cosine", num_warmup_steps=2, num_training_steps=STEPS, nonfinite="skip", step_log=4)
    eager, user_keys = make(kind, optim, **opts)
    replayed, _ = make(kind, optim, **opts)
    poison(eager, user_keys, bad_user)
    poison(replayed, user_keys, bad_user)
    static = replayed.capture(BATCH)
    assert same_state(replayed, eager) and replayed.step_counters() == {"attempts": 0, "skipped": 0, "skipped_in_a_row": 0}
    assert replayed.step_log() == []                         # the warm-up step's counters and log row were put back
    for i, batch in enumerate(batches(kind, 5)):
        b = dev(with_user(batch, bad_user) if i == 2 else batch)
        loss = eager.step(*b).clone()
        for dst, src in zip(static[:3], b):
            dst.copy_(src)
        assert torch.equal(bits(replayed.replay()), bits(loss)) and same_state(replayed, eager)
    assert eager.step_counters() == replayed.step_counters() == {"attempts": 5, "skipped": 1, "skipped_in_a_row": 0}
    assert int(eager.step_count[0]) == 4
    assert [(r["attempt"], r["opt_step"], r["skipped"], r["lr"]) for r in eager.step_log()] == \
        [(r["attempt"], r["opt_step"], r["skipped"], r["lr"]) for r in replayed.step_log()]
    assert [r["attempt"] for r in eager.step_log()] == [1, 2, 3, 4]      # a ring of 4


# ---- the state --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("optim", ["adamw", "sgd"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_state_round_trip_changes_nothing(kind, optim):
    opts = dict(scheduler_type="polynomial", num_warmup_steps=2, num_training_steps=STEPS, nonfinite="skip", step_log=4)
    straight, _ = make(kind, optim, **opts)
    first, _ = make(kind, optim, **opts)
    second, _ = make(kind, optim, **opts)
    bs = batches(kind, 6)
    for b in bs:
        straight.step(*dev(b))
    for b in bs[:3]:
        first.step(*dev(b))
    sd = first.state_dict()
    assert ("exp_avg" in sd) == ("exp_avg_sq" in sd) == (optim == "adamw")
    assert sd["optim"] == optim and sd["schedule"] == ("polynomial", 2, STEPS) and sd["step_counters"].tolist() == [3, 0, 0, 0]
    second.load_state_dict(sd)
    assert second.step_log() == first.step_log() and len(second.step_log()) == 3
    for b in bs[3:]:
        second.step(*dev(b))
    assert same_state(second, straight) and second.step_log() == straight.step_log() and second.step_counters() == straight.step_counters()


@pytest.mark.parametrize("kind", KINDS)
def test_states_of_another_optimizer_or_schedule_are_refused_and_a_state_without_the_keys_loads(kind):
    adamw, _ = make(kind)
    sgd, _ = make(kind, "sgd")
    assert sgd.exp_avg is None and sgd.exp_avg_sq is None and "exp_avg" not in sgd.state_dict() and "exp_avg_sq" not in sgd.state_dict()
    cosine, _ = make(kind, scheduler_type="cosine", num_warmup_steps=2, num_training_steps=STEPS)
    longer, _ = make(kind, scheduler_type="cosine", num_warmup_steps=2, num_training_steps=STEPS + 1)
    with pytest.raises(ValueError, match="optim = 'sgd', this trainer has 'adamw'"):
        adamw.load_state_dict(sgd.state_dict())
    with pytest.raises(ValueError, match="optim = 'adamw', this trainer has 'sgd'"):
        sgd.load_state_dict(adamw.state_dict())
    with pytest.raises(ValueError, match=r"schedule = \('cosine', 2, 20\), this trainer has None"):
        adamw.load_state_dict(cosine.state_dict())
    with pytest.raises(ValueError, match=r"schedule = \('cosine', 2, 20\), this trainer has \('cosine', 2, 21\)"):
        longer.load_state_dict(cosine.state_dict())
    # a state as the trainer wrote it before the options existed: no "optim", no "schedule"
    adamw.step(*dev(batches(kind, 1)[0]))
    old = {k: v for k, v in adamw.state_dict().items() if k not in ("optim", "schedule")}
    fresh, _ = make(kind)
    fresh.load_state_dict(old)
    assert same_state(fresh, adamw) and int(fresh.step_count[0]) == 1
    with pytest.raises(ValueError, match="optim = 'adamw', this trainer has 'sgd'"):
        sgd.load_state_dict(old)
    # what the constructor refuses
    for bad in (dict(optim="adam"), dict(nonfinite="raise"), dict(step_log=-1), dict(max_skipped_in_a_row=0), dict(scheduler_type="step"),
                dict(scheduler_type="linear"), dict(scheduler_type="linear", num_warmup_steps=-1, num_training_steps=5)):
        with pytest.raises(ValueError):
            make(kind, **bad)


def test_the_finetune_trainer_takes_none_of_the_options_and_keeps_its_state_format():
    """PmgtNcfTrainer's step is its own (pmgt_op_adamw_segments): the new keywords are a TypeError there, and its state_dict has the keys
    it had before PairTrainer's options existed."""
    from pmgt_amd.finetune import PmgtNcfTrainer
    from tests.test_finetune_step_gpu import CASES, build
    _, model = build(CASES[0])
    for kw in (dict(optim="sgd"), dict(scheduler_type="linear"), dict(nonfinite="skip"), dict(step_log=4)):
        with pytest.raises(TypeError):
            PmgtNcfTrainer(model, lr=1e-3, **kw)
    tr = PmgtNcfTrainer(model, lr=1e-3)
    sd = tr.state_dict()
    assert sorted(sd) == ["encoder", "exp_avg", "exp_avg_sq", "layout", "params", "step"]
    tr.load_state_dict(sd)
