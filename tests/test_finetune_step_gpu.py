"""PmgtNcfTrainer: fine-tuning the encoder through the NCF head on the device, on the reference's own cases (tests/golden/ncf_mlp.npz,
ncf_neumf.npz: logits, loss, encoder and head gradients of the reference's PMGT_NCF).

  * one gradient pass (trainer.grad) on an fp32 engine against the gold, at the tolerances of
    tests/test_surface_gpu.py::test_ncf_second_caller_on_hip_encoder: logits rtol 1e-4 atol 1e-5, loss rtol 1e-4, every bert.* and head
    gradient check_stored(2e-3, 2e-3 rms + 1e-8);
  * A STEP IS ITS PIECES: a second model and trainer driven by hand -- Engine.encode_train, pmgt_op_cls_gather, the rows entry,
    pmgt_op_cls_scatter, Engine.encode_backward, one pmgt_op_adamw_segments built here -- ends with the encoder's parameters, the head's, all
    moments and the step counter BIT-EQUAL to trainer.step, with and without clipping and with encoder_lr = lr / 10; what lies outside the
    encoder's ranges in the engine's buffer keeps its bits;
  * bf16 engine: err(path) = per-tensor rms difference of a path's gradient to the fp32 gold, the trainer and the autograd path of
    PMGT_NCF.forward on the same inputs; err(trainer) <= 1.5 err(autograd) + 1e-8 (both round d CLS to bf16 once and share every encoder
    kernel; only the head's fp32 rounding separates them, and 1.5 allows for flipped bf16 roundings);
  * state_dict -> three steps -> load_state_dict -> the same three steps: the same bits; no allocation in a step after reserve; the refusals.

Measured on the MI355X (one run), bf16, the largest err(trainer) / err(autograd) over the tensors: 1.000 in both cases (ncf_mlp:
predict_layer.weight 1.28e-04 / 1.28e-04, mlp_layers.2.linear.bias 9.77e-04 / 9.77e-04; ncf_neumf: predict_layer.bias 1.91e-04 / 1.91e-04,
mlp_layers.0.linear.bias 4.03e-04 / 4.03e-04): the two paths' gradients lie equally far from the fp32 gold."""
import ctypes as C

import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.configuration_pmgt import PMGTConfig
from pmgt_amd.finetune import PmgtNcfTrainer
from pmgt_amd.pmgt_ncf import PMGT_NCF
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

CASES = list(gu.NCF_CASES)


def build(name, dtype="fp32", emb_dropout=0.0, dropout=0.0):
    c = gu.ncf_case(name)
    model = PMGT_NCF(user_num=c["users"], item_num=c["n_nodes"], factor_num=c["factor"], num_layers=c["num_layers"], model=c["model"],
                     config=PMGTConfig(**c["cfg"]), dtype=dtype, emb_dropout=emb_dropout, dropout=dropout)
    sd = model.state_dict()
    with torch.no_grad():
        for k, v in list(c["params"].items()) + list(c["head"].items()):
            sd[k].copy_(v)
        for e in model.engine.entries:                       # what is not the encoder's: something to keep
            if not e["name"].startswith("bert."):
                model.engine.view(e["name"]).normal_(generator=torch.Generator(device="cuda").manual_seed(3))
    model.set_features([t.numpy() for t in c["tables"]])
    return c, model


def batch(c):
    node_ids, mask = c["item"]["node_ids"].cuda().contiguous(), c["item"]["attention_mask"].cuda().float().contiguous()
    return c["user"].cuda(), (node_ids[:, 0] - 2).contiguous(), c["labels"].cuda().float(), node_ids, mask


def all_grads(tr):
    out = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in tr.encoder_grads().items()}
    out.update({k: v.detach().cpu().numpy().astype(np.float64) for k, v in tr.views(tr.grads).items()})
    return out


@pytest.mark.parametrize("name", CASES)
def test_one_gradient_pass_equals_the_reference(name):
    c, model = build(name)
    gold = c["gold"]
    tr = PmgtNcfTrainer(model, lr=1e-3)
    tr.enc_grads.fill_(float("nan"))                         # the ranges the backward owns are written whole ...
    loss, logits = tr.grad(*batch(c))
    np.testing.assert_allclose(logits.cpu().numpy(), gold["logits"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(loss.item(), gold["loss"], rtol=1e-4)
    grads = all_grads(tr)
    assert set(grads) == {k for k, p in model.named_parameters() if p.requires_grad}
    bad = []
    for k, g in grads.items():
        assert np.isfinite(g).all(), k
        try:
            gu.check_stored(gold, "grad/" + k, g, 2e-3, 2e-3 * float(np.sqrt((g ** 2).mean())) + 1e-8)
        except AssertionError as e:
            bad.append((k, str(e).splitlines()[3:6]))
    assert not bad, bad
    outside = torch.ones_like(tr.enc_grads, dtype=torch.bool)
    for lo, hi in tr.segments:
        outside[lo:hi] = False
    assert outside.any() and torch.isnan(tr.enc_grads[outside]).all()      # ... and nothing else is


def hand_step(model, tr, b, max_norm, lr_scale):
    """trainer.step restated call by call over `tr`'s buffers: the engine's own Python entries, the two glue ops, the rows entry and ONE
    segmented optimizer call whose segment list is built here"""
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
    segs = (_lib.AdamSegmentC * (len(tr.segments) + 1))()
    for k, (lo, hi) in enumerate(tr.segments):
        segs[k] = _lib.AdamSegmentC(eng.params[lo:hi].data_ptr(), tr.enc_grads[lo:hi].data_ptr(), tr.enc_exp_avg[k].data_ptr(),
                                    tr.enc_exp_avg_sq[k].data_ptr(), eng.decay_mask[lo:hi].data_ptr(), hi - lo, lr_scale)
    segs[len(tr.segments)] = _lib.AdamSegmentC(tr.params.data_ptr(), tr.grads.data_ptr(), tr.exp_avg.data_ptr(), tr.exp_avg_sq.data_ptr(),
                                               tr.decay.data_ptr(), tr.count, 1.0)
    part, scal = torch.zeros(1024 * len(segs), device="cuda"), torch.zeros(8, device="cuda")
    _lib.check(lib.pmgt_op_adamw_segments(segs, len(segs), tr.lr, tr.weight_decay, tr.betas[0], tr.betas[1], tr.eps, max_norm,
                                          tr.step_count.data_ptr(), scal.data_ptr(), part.data_ptr(), st))
    return loss, scal


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("max_norm,enc_ratio", [(None, None), (0.05, None), (0.05, 0.1)], ids=["noclip", "clip", "clip-enc_lr"])
def test_a_step_is_its_pieces(name, max_norm, enc_ratio):
    lr, wd = 1e-3, 0.01
    kw = dict(lr=lr, weight_decay=wd, max_grad_norm=max_norm, encoder_lr=None if enc_ratio is None else lr * enc_ratio)
    (c, model_a), (_, model_b) = build(name), build(name)
    tr_a, tr_b = PmgtNcfTrainer(model_a, **kw), PmgtNcfTrainer(model_b, **kw)
    assert tr_a.lr_scale == (1.0 if enc_ratio is None else float(lr * enc_ratio) / float(lr))
    b = batch(c)
    outside_before = model_a.engine.params.clone()
    for t in (1, 2):
        loss_a = tr_a.step(*b).clone()
        loss_b, scal = hand_step(model_b, tr_b, b, float(max_norm or 0.0), tr_b.lr_scale)
        torch.cuda.synchronize()
        assert int(tr_a.step_count[0]) == t == int(tr_b.step_count[0])
        assert torch.equal(loss_a, loss_b)
        assert torch.equal(tr_a._scal[:4], scal[:4])
        if max_norm:
            assert float(scal[0]) < 1.0                      # the clip is active: the gradient norm of these cases is above 0.05
        eq = lambda x, y: torch.equal(x.view(torch.int32), y.view(torch.int32))
        assert eq(model_a.engine.params, model_b.engine.params) and eq(tr_a.params, tr_b.params)
        assert eq(tr_a.exp_avg, tr_b.exp_avg) and eq(tr_a.exp_avg_sq, tr_b.exp_avg_sq)
        for x, y in zip(tr_a.enc_exp_avg + tr_a.enc_exp_avg_sq, tr_b.enc_exp_avg + tr_b.enc_exp_avg_sq):
            assert eq(x, y)
    # the step moved the encoder and the head, and nothing outside the encoder's ranges
    moved = model_a.engine.params != outside_before
    inside = torch.zeros_like(moved)
    for lo, hi in tr_a.segments:
        inside[lo:hi] = True
    assert moved[inside].float().mean() > 0.5 and not moved[~inside].any() and (~inside).sum() > 0
    assert all(torch.equal(p, tr_a.views(tr_a.params)[k]) for k, p in model_a.named_parameters() if k in tr_a.layout)      # the model sees the head
    assert int(model_a.engine.opt_step[0]) == 0 and model_a.engine.exp_avg is None      # the engine's own optimizer state is not used


def gold_rms_diff(gold, key, arr):
    a = np.asarray(arr, dtype=np.float64)
    if key in gold.files:
        return float(np.sqrt(((a - gold[key]) ** 2).mean()))
    return float(np.sqrt(((a.ravel()[::gu.STRIDE] - gold[key + "@strided"]) ** 2).mean()))


@pytest.mark.parametrize("name", CASES)
def test_bf16_gradients_are_as_close_to_the_gold_as_autograds(name):
    (c, model_t), (_, model_g) = build(name, "bf16"), build(name, "bf16")
    gold = c["gold"]
    tr = PmgtNcfTrainer(model_t, lr=1e-3)
    tr.grad(*batch(c))
    got = all_grads(tr)
    model_g.train()
    logits = model_g(c["user"], c["item"])
    torch.nn.functional.binary_cross_entropy_with_logits(logits, c["labels"].cuda()).backward()
    auto = {k: p.grad.cpu().numpy().astype(np.float64) for k, p in model_g.named_parameters() if p.requires_grad}
    assert set(auto) == set(got)
    rows, bad = [], []
    for k in got:
        e_t, e_a = gold_rms_diff(gold, "grad/" + k, got[k]), gold_rms_diff(gold, "grad/" + k, auto[k])
        rows.append((e_t / e_a if e_a > 0 else float(e_t > 0), k, e_t, e_a))
        if not e_t <= 1.5 * e_a + 1e-8:
            bad.append((k, e_t, e_a))
    rows.sort(reverse=True)
    print(f"{name} bf16, err(trainer) / err(autograd), the five largest: " + ", ".join(f"{k} {r:.3f} ({a:.2e} / {b:.2e})" for r, k, a, b in rows[:5]))
    assert not bad, bad


def test_state_roundtrip_and_no_allocation_in_a_step():
    c, model = build("ncf_neumf", emb_dropout=0.2, dropout=0.1)
    tr = PmgtNcfTrainer(model, lr=1e-3, weight_decay=0.01, max_grad_norm=1.0, dropout_seed=5, check_carrier_every=3)
    assert tr.step_count.data_ptr() == tr.rng[1:].data_ptr()      # the one step counter is the mask stream's step
    b = batch(c)
    tr.reserve(len(b[0]), b[3].shape[1])
    loss = torch.zeros(1, device="cuda")
    tr.step(*b, loss=loss)                                   # (loads the kernels)
    torch.cuda.synchronize()
    before = torch.cuda.memory_stats()["allocation.all.allocated"]
    tr.step(*b, loss=loss)
    torch.cuda.synchronize()
    assert torch.cuda.memory_stats()["allocation.all.allocated"] == before      # (the carrier guard, every third step here, is not in it)
    sd = tr.state_dict()
    snap = lambda: [t.clone() for t in [model.engine.params, tr.params, tr.exp_avg, tr.exp_avg_sq, tr.step_count, model.engine.rng_state]
                    + tr.enc_exp_avg + tr.enc_exp_avg_sq]
    losses = [tr.step(*b).clone() for _ in range(3)]
    first = snap()
    tr.load_state_dict(sd)
    assert int(tr.step_count[0]) == 2
    again = [tr.step(*b).clone() for _ in range(3)]
    for x, y in zip(first + losses, snap() + again):
        assert torch.equal(x, y)
    assert len({float(x) for x in losses}) == 3              # fresh masks every step
    # another seed, another layout: refused
    with pytest.raises(ValueError, match="dropout_seed"):
        tr.load_state_dict(dict(sd, dropout_seed=6))
    with pytest.raises(ValueError, match="layouts differ"):
        tr.load_state_dict(dict(sd, encoder=dict(sd["encoder"], segments=[(0, 8)])))
    with pytest.raises(ValueError, match="layouts differ"):
        tr.load_state_dict({k: v for k, v in sd.items() if k != "encoder"})
    with pytest.raises(NotImplementedError):
        tr.capture(4)


def test_the_layernorm_carrier_guard_runs_every_n_steps_and_after_a_load():
    """The encoder's LayerNorm parameters move under this trainer, so the guard of Trainer._check_carrier runs here: |beta / gamma| pushed
    past the bound behind the engine's back is seen at the next multiple of check_carrier_every, and by load_state_dict at once."""
    import warnings
    c, model = build("ncf_mlp")
    eng = model.engine
    tr = PmgtNcfTrainer(model, lr=1e-4, check_carrier_every=2)
    b = batch(c)
    sd = tr.state_dict()
    tr.step(*b)
    eng.view("bert.encoder.layer.0.output.LayerNorm.bias").fill_(20.0)
    assert not eng.get_option("store_ln_input")
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        tr.step(*b)                                          # step 2: the guard looks
    assert eng.get_option("store_ln_input") and any("store_ln_input" in str(w.message) for w in seen)
    tr.step(*b)                                              # the workspace is carved for the new option: the step goes on
    torch.cuda.synchronize()
    assert torch.isfinite(eng.params).all() and torch.isfinite(tr.params).all()
    eng.set_option("store_ln_input", 0)
    sd["encoder"]["params"][0][eng.entry("bert.encoder.layer.1.output.LayerNorm.bias")["offset"] - tr.segments[0][0]] = 30.0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tr.load_state_dict(sd)
    assert eng.get_option("store_ln_input") and int(tr.step_count[0]) == 0


def test_refusals():
    c, model = build("ncf_mlp")
    for attr, value, match in (("factor_num", 12, "factor_num"), ("num_layers", 2, "hidden_size"), ("model", "GMF", "kind")):
        keep = getattr(model, attr)
        setattr(model, attr, value)
        with pytest.raises(ValueError, match=match):
            PmgtNcfTrainer(model)
        setattr(model, attr, keep)
    model.emb_dropout.p = 0.1
    with pytest.raises(ValueError, match="dropout_seed"):
        PmgtNcfTrainer(model)
    with pytest.raises(ValueError, match="dropout_seed"):
        PmgtNcfTrainer(model, dropout_seed=1.5)
    model.emb_dropout.p = 0.0
    for bad in (-1e-4, float("nan"), float("inf"), "1e-4"):
        with pytest.raises(ValueError, match="encoder_lr"):
            PmgtNcfTrainer(model, encoder_lr=bad)
    with pytest.raises(ValueError, match="encoder_lr"):
        PmgtNcfTrainer(model, lr=0.0, encoder_lr=1e-4)
    head_before = {k: v.clone() for k, v in model.state_dict().items()}
    tr = PmgtNcfTrainer(model, encoder_lr=0.0)               # a frozen encoder is a rate like any other
    assert all(torch.equal(v, head_before[k]) for k, v in model.state_dict().items())      # adopting the head moves no value
    users, items, labels, node_ids, mask = batch(c)
    n, S = node_ids.shape
    bad = [dict(node_ids=node_ids[:-1]), dict(node_ids=node_ids.int()), dict(node_ids=node_ids.cpu()), dict(attention_mask=mask.double()),
           dict(attention_mask=mask[:, :-1]), dict(attention_mask=mask.cpu()), dict(node_ids=node_ids.t()),
           dict(users=users[:0], items=items[:0], labels=labels[:0], node_ids=node_ids[:0], attention_mask=mask[:0]),
           dict(users=users.int()), dict(labels=labels.double()), dict(items=items[:-1])]
    big = 65537
    bad.append(dict(users=torch.zeros(big, dtype=torch.int64, device="cuda"), items=torch.zeros(big, dtype=torch.int64, device="cuda"),
                    labels=torch.zeros(big, device="cuda"), node_ids=torch.full((big, S), 2, dtype=torch.int64, device="cuda"),
                    attention_mask=torch.ones(big, S, device="cuda")))
    params_before, head_before = model.engine.params.clone(), tr.params.clone()
    for kw in bad:
        args = dict(users=users, items=items, labels=labels, node_ids=node_ids, attention_mask=mask)
        args.update(kw)
        with pytest.raises(ValueError):
            tr.step(**args)
    with pytest.raises(ValueError, match="outside"):
        tr.reserve(0)
    torch.cuda.synchronize()
    assert torch.equal(model.engine.params, params_before) and torch.equal(tr.params, head_before) and int(tr.step_count[0]) == 0
    tr.step(users, items, labels, node_ids, mask)            # and the well-formed call goes through
    torch.cuda.synchronize()
    assert int(tr.step_count[0]) == 1 and torch.equal(model.engine.params, params_before) and not torch.equal(tr.params, head_before)
