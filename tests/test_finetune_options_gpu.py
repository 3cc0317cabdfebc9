"""PmgtNcfOptionsTrainer: PmgtNcfTrainer with PairTrainer's options -- SGD, a learning-rate schedule, the step guard -- and the whole step as one graph, on the cases
and with the fixtures of tests/test_finetune_step_gpu.py (ncf_mlp, ncf_neumf).

  * A default-keyword trainer's state has exactly the keys it always had.
  * A STEP WITH OPTIONS IS ITS PIECES: a second model and trainer driven by hand, ending in one pmgt_op_step_segments built here, ends with
    the encoder's parameters, the head's, all moments, the step counter and the guard's state BIT-EQUAL to trainer.step; what lies outside
    the encoder's ranges in the engine's buffer keeps its bits.
  * The guard end to end: a batch that meets an Inf embedding row is skipped -- engine.params WHOLE, the head, all moments and the step keep
    their bits, engine.rng_state has advanced --, the next batch applies, two skips in a row raise, and the logged rates are the schedule's.
  * SGD holds no moments, in the trainer or in its state; the state round trip; a state of another optimizer or schedule is refused by name.
  * capture_step leaves the state as it was; replays on different batches (one skipped), and eager and replayed steps mixed, are a twin
    trainer's eager steps bit for bit; the carrier flip under replay re-captures and goes on as the eager twin does."""
import ctypes as C
import warnings

import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.finetune import PmgtNcfOptionsTrainer, PmgtNcfTrainer
from pmgt_amd.trainer import NonFiniteGradientsError
from tests import golden_util as gu
from tests.test_finetune_step_gpu import CASES, batch, build

pytestmark = pytest.mark.gpu

LR, WD = 1e-3, 0.01


def build_with(name, hidden_dropout=0.0, **kw):
    """build() of tests/test_finetune_step_gpu.py on the case's config with the encoder's dropout set"""
    real = gu.ncf_case

    def case(n):
        c = real(n)
        c["cfg"]["hidden_dropout_prob"] = hidden_dropout
        return c
    gu.ncf_case = case
    try:
        return build(name, **kw)
    finally:
        gu.ncf_case = real


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def snapshot(model, tr):
    """everything a step may move, cloned: engine.params WHOLE, the head, all moments, the step, engine.rng_state, the guard's state"""
    moments = ([tr.exp_avg, tr.exp_avg_sq] if tr.exp_avg is not None else []) + tr.enc_exp_avg + tr.enc_exp_avg_sq
    guard = [] if tr._guard_state is None else [tr._guard_state]
    return dict(encoder=model.engine.params.clone(), head=tr.params.clone(), moments=[m.clone() for m in moments], step=tr.step_count.clone(),
                rng=model.engine.rng_state.clone(), guard=[g.clone() for g in guard])


def assert_same(a, b, skip=()):
    for k in a:
        if k in skip:
            continue
        xs, ys = (a[k], b[k]) if isinstance(a[k], list) else ([a[k]], [b[k]])
        assert len(xs) == len(ys), k
        for x, y in zip(xs, ys):
            assert torch.equal(bits(x), bits(y)), k


def variant(c, k, with_user=None, without_user=None):
    """batch k of a case: the contexts rolled by k rows (the items with them), the users by 2 k, every other label flipped for odd k;
    with_user: that user at position 0; without_user: that user replaced everywhere"""
    users, _, labels, node_ids, mask = batch(c)
    node_ids, mask = node_ids.roll(k, 0).contiguous(), mask.roll(k, 0).contiguous()
    users, labels = users.roll(2 * k).contiguous(), labels.clone()
    if k % 2:
        labels[::2] = 1.0 - labels[::2]
    if without_user is not None:
        users[users == without_user] = (without_user + 1) % c["users"]
    if with_user is not None:
        users[0] = with_user
    return users, (node_ids[:, 0] - 2).contiguous(), labels, node_ids, mask


@pytest.mark.parametrize("cls", [PmgtNcfTrainer, PmgtNcfOptionsTrainer])
@pytest.mark.parametrize("seed", [None, 5])
def test_a_default_trainer_keeps_the_state_it_always_had(seed, cls):
    c, model = build("ncf_mlp", emb_dropout=0.0 if seed is None else 0.2)
    tr = cls(model, lr=LR, dropout_seed=seed)
    want = {"params", "step", "layout", "exp_avg", "exp_avg_sq", "encoder"} | ({"dropout_seed"} if seed is not None else set())
    assert set(tr.state_dict()) == want
    assert set(tr.state_dict()["encoder"]) == {"segments", "params", "exp_avg", "exp_avg_sq", "rng_state", "dtype"}
    assert tr.schedule() is None and tr.step_counters() is None and tr.step_log() == [] and tr.check_nonfinite() is None


def hand_step(model, tr, b, max_norm, lr_scale, optim, sched, guard_rows, skip):
    """trainer.step restated call by call over `tr`'s buffers: the engine's own Python entries, the two glue ops, the rows entry and ONE
    pmgt_op_step_segments whose segment list, schedule and guard are built here"""
    users, items, labels, node_ids, mask = b
    eng, lib, st = model.engine, _lib.hip(), _lib.stream()
    n, S = node_ids.shape
    d = model.config.hidden_size
    last, state = eng.encode_train(ids=node_ids, attention_mask=mask, training=True)
    x = torch.empty(n, d, device="cuda")
    _lib.check(lib.pmgt_op_cls_gather(eng.dtype_code, last.data_ptr(), n, S, d, x.data_ptr(), st))
    d_item = torch.empty(n, d, device="cuda")
    tr.grad_fn.bind(x, d_item)
    loss, _ = tr.grad_fn(users, items, labels)
    d_last = torch.full((n, S, d), float("nan"), device="cuda", dtype=eng.torch_dtype)
    _lib.check(lib.pmgt_op_cls_scatter(eng.dtype_code, d_item.data_ptr(), n, S, d, d_last.data_ptr(), st))
    eng.encode_backward(state, d_last, grad_buffer=tr.enc_grads)
    adam = optim == "adamw"                                  # (SGD: no moments exist, the segments' m and v are NULL)
    segs = (_lib.AdamSegmentC * (len(tr.segments) + 1))()
    for k, (lo, hi) in enumerate(tr.segments):
        segs[k] = _lib.AdamSegmentC(eng.params[lo:hi].data_ptr(), tr.enc_grads[lo:hi].data_ptr(), tr.enc_exp_avg[k].data_ptr() if adam else None,
                                    tr.enc_exp_avg_sq[k].data_ptr() if adam else None, eng.decay_mask[lo:hi].data_ptr(), hi - lo, lr_scale)
    segs[len(tr.segments)] = _lib.AdamSegmentC(tr.params.data_ptr(), tr.grads.data_ptr(), tr.exp_avg.data_ptr() if adam else None,
                                               tr.exp_avg_sq.data_ptr() if adam else None, tr.decay.data_ptr(), tr.count, 1.0)
    part, scal = torch.zeros(1024 * len(segs), device="cuda"), torch.zeros(8, device="cuda")
    sc = _lib.LrScheduleC(_lib.LR_SCHEDULE_TYPES.index(sched[0]), sched[1], sched[2])
    gd = None
    if tr._guard_state is not None:                          # counters [4], log_i [R][2], log_f [R][STEP_LOG_FLOATS], in one int64 buffer
        base = tr._guard_state.data_ptr()
        gd = C.byref(_lib.StepGuardC(base, base + 8 * (4 + 2 * guard_rows), base + 32, guard_rows, loss.data_ptr(), skip))
    _lib.check(lib.pmgt_op_step_segments(segs, len(segs), _lib.OPTIMS.index(optim), tr.lr, tr.weight_decay, tr.betas[0], tr.betas[1], tr.eps,
                                         max_norm, tr.step_count.data_ptr(), scal.data_ptr(), part.data_ptr(), C.byref(sc), gd, st))
    return loss, scal


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("max_norm,enc_ratio", [(0.05, None), (0.05, 0.1)], ids=["clip", "clip-enc_lr"])
@pytest.mark.parametrize("optim,sched,guard", [("sgd", ("linear", 1, 6), None), ("adamw", ("cosine", 1, 6), dict(nonfinite="skip", step_log=4))],
                         ids=["sgd-linear", "adamw-cosine-guard"])
def test_a_step_with_options_is_its_pieces(name, max_norm, enc_ratio, optim, sched, guard):
    kw = dict(lr=LR, weight_decay=WD, max_grad_norm=max_norm, encoder_lr=None if enc_ratio is None else LR * enc_ratio, optim=optim,
              scheduler_type=sched[0], num_warmup_steps=sched[1], num_training_steps=sched[2], **(guard or {}))
    (c, model_a), (_, model_b) = build(name), build(name)
    tr_a, tr_b = PmgtNcfOptionsTrainer(model_a, **kw), PmgtNcfOptionsTrainer(model_b, **kw)
    assert tr_a.schedule() == sched and (tr_a._guard_state is not None) == (guard is not None)
    b = batch(c)
    outside_before = model_a.engine.params.clone()
    for t in (1, 2, 3):
        loss_a = tr_a.step(*b).clone()
        loss_b, scal = hand_step(model_b, tr_b, b, max_norm, tr_b.lr_scale, optim, sched, 4 if guard else 0, 1)
        torch.cuda.synchronize()
        assert int(tr_a.step_count[0]) == t == int(tr_b.step_count[0]) and torch.equal(loss_a, loss_b)
        assert torch.equal(bits(tr_a._scal[:5]), bits(scal[:5])) and float(scal[0]) < 1.0      # the clip is active
        assert_same(snapshot(model_a, tr_a), snapshot(model_b, tr_b))
    if guard:
        assert tr_a.step_counters() == dict(attempts=3, skipped=0, skipped_in_a_row=0) and [r["opt_step"] for r in tr_a.step_log()] == [1, 2, 3]
    moved = model_a.engine.params != outside_before
    inside = torch.zeros_like(moved)
    for lo, hi in tr_a.segments:
        inside[lo:hi] = True
    assert moved[inside].any() and not moved[~inside].any() and (~inside).sum() > 0


@pytest.mark.parametrize("name", CASES)
def test_the_guard_end_to_end(name):
    sched = ("linear", 1, 6)
    c, model = build_with(name, hidden_dropout=0.1)
    tr = PmgtNcfOptionsTrainer(model, lr=LR, weight_decay=WD, max_grad_norm=0.05, scheduler_type=sched[0], num_warmup_steps=sched[1],
                        num_training_steps=sched[2], nonfinite="skip", step_log=16, max_skipped_in_a_row=2)
    poisoned = int(batch(c)[0][0])
    views = tr.views(tr.params)
    for key in ("mlp_user_embeddings.weight", "gmf_user_embeddings.weight"):
        if key in views:
            views[key][poisoned] = float("inf")
    bad, good = variant(c, 0, with_user=poisoned), variant(c, 1, without_user=poisoned)
    before = snapshot(model, tr)
    losses = [tr.step(*bad).clone()]
    torch.cuda.synchronize()
    after = snapshot(model, tr)
    assert_same(before, after, skip=("rng", "guard"))        # engine.params WHOLE, the head, every moment, the step counter
    assert not torch.equal(before["rng"], after["rng"])      # the forward ran: the encoder's dropout counter has advanced
    assert tr.check_nonfinite() == dict(attempts=1, skipped=1, skipped_in_a_row=1) and float(tr._scal[5]) == 1.0
    losses.append(tr.step(*good).clone())                    # a batch without the user applies
    torch.cuda.synchronize()
    assert int(tr.step_count[0]) == 1 and tr.check_nonfinite() == dict(attempts=2, skipped=1, skipped_in_a_row=0)
    assert not torch.equal(snapshot(model, tr)["encoder"], after["encoder"]) or float(tr._scal[4]) == 0.0      # (step 0 of the warm-up runs at rate 0)
    losses += [tr.step(*bad).clone(), tr.step(*bad).clone()]
    with pytest.raises(NonFiniteGradientsError, match="2 optimizer steps in a row"):
        tr.check_nonfinite()
    norms = []
    for k in range(5):                                       # applied steps 2 .. 6
        losses.append(tr.step(*variant(c, k, without_user=poisoned)).clone())
        norms.append(tr.grad_norm().clone())
    torch.cuda.synchronize()
    assert not torch.equal(snapshot(model, tr)["encoder"], after["encoder"])
    log = tr.step_log()
    assert [r["attempt"] for r in log] == list(range(9)) and [r["skipped"] for r in log] == [True, False, True, True] + [False] * 5
    assert [r["opt_step"] for r in log] == [0, 1, 1, 1, 2, 3, 4, 5, 6] and [r["nonfinite"] for r in log] == [r["skipped"] for r in log]
    want = torch.zeros(7, device="cuda")
    sc = _lib.LrScheduleC(_lib.LR_SCHEDULE_TYPES.index(sched[0]), sched[1], sched[2])
    _lib.check(_lib.hip().pmgt_op_lr_schedule(C.byref(sc), tr.lr, 0, 7, want.data_ptr(), _lib.stream()))
    applied = [r for r in log if not r["skipped"]]
    assert [r["lr"] for r in applied] == [float(x) for x in want[:6].cpu()] and applied[1]["lr"] == float(torch.tensor(LR, dtype=torch.float32))
    assert [r["lr"] for r in log if r["skipped"]] == [float(want[0]), float(want[1]), float(want[1])]      # the rate it would have used
    for r, loss in zip(log, losses):
        assert (r["loss"] == float(loss)) or (r["skipped"] and r["loss"] != r["loss"] and float(loss) != float(loss))      # the step's own loss
        assert (r["clip_coef"] == 0.0 and not r["grad_norm"] < float("inf")) if r["skipped"] else 0.0 < r["clip_coef"] < 1.0
    assert [r["grad_norm"] for r in applied[1:]] == [float(x) for x in norms]


@pytest.mark.parametrize("name", CASES)
def test_sgd_holds_no_moments_and_its_state_round_trips(name):
    c, model = build_with(name, hidden_dropout=0.1, emb_dropout=0.2, dropout=0.1)
    kw = dict(lr=0.05, weight_decay=WD, max_grad_norm=1.0, dropout_seed=5, optim="sgd", scheduler_type="linear", num_warmup_steps=1, num_training_steps=9)
    tr = PmgtNcfOptionsTrainer(model, **kw)
    assert tr.exp_avg is None and tr.exp_avg_sq is None and tr.enc_exp_avg == [] and tr.enc_exp_avg_sq == []
    b = [variant(c, k) for k in range(3)]
    tr.step(*b[0])
    sd = tr.state_dict()
    assert sd["optim"] == "sgd" and sd["schedule"] == ("linear", 1, 9) and "step_counters" not in sd
    assert not {"exp_avg", "exp_avg_sq"} & set(sd) and not {"exp_avg", "exp_avg_sq"} & set(sd["encoder"])
    losses = [tr.step(*x).clone() for x in b]
    first = snapshot(model, tr)
    tr.load_state_dict(sd)
    assert int(tr.step_count[0]) == 1
    again = [tr.step(*x).clone() for x in b]
    assert_same(first, snapshot(model, tr))
    assert all(torch.equal(x, y) for x, y in zip(losses, again))
    assert not torch.equal(first["head"], sd["params"]) and not torch.equal(first["rng"], sd["encoder"]["rng_state"])
    # a state saved under another optimizer or schedule is refused by name, with nothing written
    keep = snapshot(model, tr)
    _, other = build_with(name, hidden_dropout=0.1, emb_dropout=0.2, dropout=0.1)
    for kw2, word in ((dict(kw, optim="adamw"), "optim = 'adamw'"), (dict(kw, scheduler_type="cosine"), "schedule = \\('cosine', 1, 9\\)"),
                      ({k: v for k, v in kw.items() if k not in ("optim", "scheduler_type", "num_warmup_steps", "num_training_steps")},
                       "optim = 'adamw'")):
        theirs = PmgtNcfOptionsTrainer(other, **kw2).state_dict()
        with pytest.raises(ValueError, match=word):
            tr.load_state_dict(theirs)
    with pytest.raises(ValueError, match="schedule = None"):
        tr.load_state_dict({k: v for k, v in dict(sd).items() if k != "schedule"})
    assert_same(keep, snapshot(model, tr))


def feed(static, b):
    for buf, t in zip(static, b):
        buf.copy_(t)


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("kw", [dict(optim="adamw", scheduler_type="cosine", num_warmup_steps=1, num_training_steps=12, nonfinite="skip", step_log=4,
                                     weight_decay=WD),
                                dict(optim="sgd", nonfinite="skip", lr=0.05)], ids=["adamw-cosine-guard", "sgd-guard"])
def test_replayed_steps_are_a_twins_eager_steps(name, kw):
    kw = dict(dict(lr=LR, max_grad_norm=1.0, dropout_seed=5), **kw)
    (c, model_a), (_, model_b) = (build_with(name, hidden_dropout=0.1, emb_dropout=0.2, dropout=0.1) for _ in range(2))
    tr_a, tr_b = PmgtNcfOptionsTrainer(model_a, **kw), PmgtNcfOptionsTrainer(model_b, **kw)
    poisoned = c["users"] - 1
    for tr in (tr_a, tr_b):
        views = tr.views(tr.params)
        for key in ("mlp_user_embeddings.weight", "gmf_user_embeddings.weight"):
            if key in views:
                views[key][poisoned] = float("inf")
    batches = [variant(c, k, without_user=poisoned) for k in range(4)]
    batches[2] = variant(c, 2, with_user=poisoned)
    n, S = batches[0][3].shape
    with pytest.raises(NotImplementedError, match="capture_step"):
        tr_a.capture(4)
    live = model_a.engine._live_graphs
    before = snapshot(model_a, tr_a)
    static = tr_a.capture_step(n, S)
    torch.cuda.synchronize()
    assert_same(before, snapshot(model_a, tr_a))             # capturing leaves the state as it was, engine.rng_state and the guard included
    assert model_a.engine._live_graphs == live + 1 and len(static) == 6
    for k, b in enumerate(batches):                          # four replays on four different batches, the third skipped
        feed(static, b)
        loss_a = tr_a.replay_step().clone()
        loss_b = tr_b.step(*b).clone()
        assert torch.equal(bits(loss_a), bits(loss_b)) or k == 2, k
        assert_same(snapshot(model_a, tr_a), snapshot(model_b, tr_b))
    assert tr_a.step_counters() == dict(attempts=4, skipped=1, skipped_in_a_row=0) == tr_b.step_counters() and int(tr_a.step_count[0]) == 3
    for k, eager in ((1, True), (0, False), (3, True), (2, False), (1, False)):      # eager and replayed steps interleaved
        if eager:
            tr_a.step(*batches[k])
        else:
            feed(static, batches[k])
            tr_a.replay_step()
        tr_b.step(*batches[k])
        assert_same(snapshot(model_a, tr_a), snapshot(model_b, tr_b))
    assert tr_a.step_counters() == dict(attempts=9, skipped=2, skipped_in_a_row=0) and int(tr_a.step_count[0]) == 7
    assert not torch.equal(before["encoder"], model_a.engine.params)
    tr_a._drop_graph()
    assert model_a.engine._live_graphs == live


def carrier_world():
    """a bf16 engine at hidden size 256 under the head (64, 3, NeuMF-end): 1 layer, 8 heads; 8 pairs with contexts of 8 tokens"""
    from pmgt_amd.configuration_pmgt import PMGTConfig
    from pmgt_amd.models import synthetic_features
    from pmgt_amd.pmgt_ncf import PMGT_NCF
    n_items, n_users, n, S = 40, 12, 8, 8
    torch.manual_seed(0)
    cfg = PMGTConfig(hidden_size=256, num_hidden_layers=1, num_attention_heads=8, intermediate_size=256, feat_hidden_sizes=(32, 16),
                     hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = PMGT_NCF(user_num=n_users, item_num=n_items, factor_num=64, num_layers=3, model="NeuMF-end", config=cfg, dtype="bf16")
    model.set_features(synthetic_features(n_items, (32, 16), seed=1))
    gen = torch.Generator().manual_seed(2)
    batches = []
    for _ in range(3):
        node_ids = torch.randint(2, n_items + 2, (n, S), generator=gen)
        batches.append((torch.randint(0, n_users, (n,), generator=gen).cuda(), (node_ids[:, 0] - 2).cuda(),
                        torch.randint(0, 2, (n,), generator=gen).float().cuda(), node_ids.cuda(), torch.ones(n, S).cuda()))
    return model, batches


def test_the_carrier_flip_under_replay_recaptures_and_steps_on():
    (model_a, batches), (model_b, _) = carrier_world(), carrier_world()
    kw = dict(lr=LR, max_grad_norm=1.0, check_carrier_every=1)
    tr_a, tr_b = PmgtNcfTrainer(model_a, **kw), PmgtNcfTrainer(model_b, **kw)      # (all defaults: the plain trainer captures too)
    assert torch.equal(model_a.engine.params, model_b.engine.params)
    static = tr_a.capture_step(8, 8)
    feed(static, batches[0])
    tr_a.replay_step()
    tr_b.step(*batches[0])
    assert_same(snapshot(model_a, tr_a), snapshot(model_b, tr_b))
    for eng in (model_a.engine, model_b.engine):
        eng.view("bert.encoder.layer.0.output.LayerNorm.bias").fill_(20.0)      # |beta / gamma| = 20 > 8, behind the engine's back
        assert not eng.get_option("store_ln_input")
    feed(static, batches[1])
    with pytest.warns(UserWarning, match="store_ln_input"):
        tr_a.replay_step()                                   # warns, switches the option, re-captures over the SAME static buffers
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tr_b.step(*batches[1])
    assert model_a.engine.get_option("store_ln_input") and model_b.engine.get_option("store_ln_input") and model_a.engine._live_graphs == 1
    assert_same(snapshot(model_a, tr_a), snapshot(model_b, tr_b))      # the re-capture left the state as it was
    feed(static, batches[2])
    tr_a.replay_step()                                       # the new graph, under stored LayerNorm inputs
    tr_b.step(*batches[2])
    torch.cuda.synchronize()
    assert_same(snapshot(model_a, tr_a), snapshot(model_b, tr_b))
    assert int(tr_a.step_count[0]) == 3 and bool(torch.isfinite(model_a.engine.params).all())
