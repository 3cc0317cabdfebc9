"""fit_dcn and evaluate_ctr in a small synthetic world: 40 users and 120 items in 4 taste groups (user u and item i match when u % 4 ==
i % 4); every user holds 12 items of their group, 10 in the training list (400 pairs) and 2 in the validation list (80 pairs, 5 sampled
negatives each: 480 labelled pairs).  Model (16, 1, 4, LayerNorm on), E = 32, batches of 64, num_ng 1, clipping at 5, AdamW.

LR AND EPOCH COUNT were chosen on the CPU with the torch yardstick of the same procedure (torch_fit below: ng_sample, epoch_order,
pmgt_amd.dcn.DCN in fp32 torch, autograd, clip_grad_norm_, AdamW with the reference's groups) over lr in {1e-2, 3e-2} and up to 50 epochs:
lr 3e-2 and 25 epochs, the smallest multiple of 5 after which no seed's best validation AUC rises any more (at lr 1e-2 the seeds still
rise at 45 epochs and end lower, 0.77 to 0.83).  The AUC levels off near 0.8 to 0.85: the validation items are new to the user, and a
sampled validation negative may be one of the user's training items.
THE BOUND on the best validation AUC comes from that fit over the torch seeds 0 .. 5 (the seed decides the model's initialisation; the
device fit starts from seed 0's): the worst seed minus the spread (max - min),
    seed       0       1       2       3       4       5
    first      0.5019  0.5170  0.4948  0.4920  0.4896  0.4825      (the AUC after epoch 0)
    best       0.8074  0.8397  0.8186  0.8201  0.8308  0.8453
    bound = min - (max - min) = 0.8074 - 0.0379 = 0.7695
(python -m tests.test_fit_dcn_gpu prints them again; no GPU is needed for that.)  Measured on the MI355X (one run): the device fit's
validation AUC went 0.4784 -> 0.7987 (the best, epoch 21), its training loss 0.7561 -> 0.1673."""
import glob
import os

import numpy as np
import pytest
import torch

from pmgt_amd.dcn import DCN
from pmgt_amd.dcn_train import validation_seed

SHAPE, USERS, ITEMS, GROUPS = (16, 1, 4, True), 40, 120, 4
EPOCHS = 25
SETTINGS = dict(batch_size=64, num_ng=1, max_sample_items=5, seed=0, lr=3e-2, weight_decay=0.0, max_grad_norm=5.0)
SEEDS = (0, 1, 2, 3, 4, 5)
SEED_BEST = (0.8074, 0.8397, 0.8186, 0.8201, 0.8308, 0.8453)      # torch seeds 0 .. 5
AUC_BOUND = min(SEED_BEST) - (max(SEED_BEST) - min(SEED_BEST))


def pair_lists():
    rng = np.random.default_rng(12)
    train, valid = [], []
    for u in range(USERS):
        own = rng.permutation(np.arange(u % GROUPS, ITEMS, GROUPS))[:12]
        train += [(u, int(i)) for i in own[:10]]
        valid += [(u, int(i)) for i in own[10:]]
    return np.asarray(train, dtype=np.int64), np.asarray(valid, dtype=np.int64)


def make_model(torch_seed):
    torch.manual_seed(torch_seed)
    return DCN(USERS, ITEMS, *SHAPE[:3], use_layer_norm=SHAPE[3], layer_norm_eps=1e-12)


def torch_fit(torch_seed, epochs=EPOCHS):
    """fit_dcn's loop on the CPU in fp32 torch -> the validation AUC after every epoch."""
    from pmgt_amd.evaluation import roc_auc_score
    from pmgt_amd.fit_loop import epoch_order
    from pmgt_amd.ncf_train import ng_sample
    train, valid = pair_lists()
    model = make_model(torch_seed).eval()
    named = list(model.named_parameters())
    opt = torch.optim.AdamW([{"params": [p for k, p in named if "bias" not in k], "weight_decay": SETTINGS["weight_decay"]},
                             {"params": [p for k, p in named if "bias" in k], "weight_decay": 0.0}], lr=SETTINGS["lr"])
    vu, vi, vl = ng_sample(valid, USERS, ITEMS, SETTINGS["max_sample_items"], validation_seed(SETTINGS["seed"]))
    aucs = []
    for epoch in range(epochs):
        users, items, labels = ng_sample(train, USERS, ITEMS, SETTINGS["num_ng"], SETTINGS["seed"] + epoch)
        order = epoch_order(len(users), SETTINGS["seed"], epoch)
        users, items, labels = (torch.from_numpy(a[order]) for a in (users, items, labels))
        for lo in range(0, len(order), SETTINGS["batch_size"]):
            hi = lo + SETTINGS["batch_size"]
            opt.zero_grad(set_to_none=True)
            torch.nn.functional.binary_cross_entropy_with_logits(model((users[lo:hi], items[lo:hi])), labels[lo:hi]).backward()
            torch.nn.utils.clip_grad_norm_([p for _, p in named if p.grad is not None], SETTINGS["max_grad_norm"])
            opt.step()
        with torch.no_grad():
            scores = torch.sigmoid(model((torch.from_numpy(vu), torch.from_numpy(vi)))).numpy()
        aucs.append(roc_auc_score(vl, scores))
    return aucs


@pytest.mark.gpu
def test_fit_learns_validates_and_keeps_the_best_parameters(tmp_path):
    from pmgt_amd import evaluate_ctr, fit_dcn
    from pmgt_amd.evaluation import roc_auc_score
    from pmgt_amd.ncf_train import ng_sample
    train, valid = pair_lists()
    model = make_model(0).cuda()
    cross_bias = model.cross_net.layers[0].bias.detach().clone()
    seen = []
    history = fit_dcn(model, train, valid, max_epochs=EPOCHS, early_criterion="auc", patience=EPOCHS, ckpt_dir=str(tmp_path), log=seen.append,
                      **SETTINGS)
    assert len(history) == EPOCHS and seen == history and [h["epoch"] for h in history] == list(range(EPOCHS))
    assert all(np.isfinite(h[k]) for h in history for k in ("train_loss", "auc", "loss")) and all(0 <= h["auc"] <= 1 for h in history)
    best = max((h for h in history if h["best"]), key=lambda h: h["epoch"])
    print("auc " + " ".join(f"{h['auc']:.4f}" for h in history) + f"; train loss {history[0]['train_loss']:.4f} -> {history[-1]['train_loss']:.4f}")
    assert best["auc"] == max(h["auc"] for h in history) and all(h["auc"] < best["auc"] for h in history[:best["epoch"]])
    assert best["auc"] >= AUC_BOUND and best["auc"] > history[0]["auc"] and best["epoch"] > 0      # it rises from the first epoch to the best
    assert history[-1]["train_loss"] < history[0]["train_loss"]
    # the best parameters are in the model and in the one checkpoint file; the unused cross bias kept its bits
    files = glob.glob(os.path.join(str(tmp_path), "*.ckpt"))
    assert [os.path.basename(f) for f in files] == [f"epoch={best['epoch']:02d}-auc={best['auc']:.4f}.ckpt"]
    ckpt = torch.load(files[0], weights_only=False)
    now = model.state_dict()
    assert ckpt["epoch"] == best["epoch"] and sorted(ckpt["state_dict"]) == sorted(now)
    assert all(torch.equal(now[k].cpu(), ckpt["state_dict"][k]) for k in now)
    assert torch.equal(model.cross_net.layers[0].bias.detach(), cross_bias)
    # the evaluation: device metrics equal host metrics; the AUC is roc_auc_score of the stored scores, exactly
    vu, vi, vl = ng_sample(valid, USERS, ITEMS, SETTINGS["max_sample_items"], validation_seed(SETTINGS["seed"]))
    on_device = evaluate_ctr(model, vu, vi, vl, batch_size=100, metrics="device")
    on_host = evaluate_ctr(model, vu, vi, vl, batch_size=100, metrics="host")
    assert on_device == on_host and on_device["n"] == len(vu) == 480
    assert on_device["auc"] == best["auc"] and on_device["loss"] == best["loss"]
    with torch.no_grad():
        logits = model((torch.from_numpy(vu).cuda(), torch.from_numpy(vi).cuda())).cpu().numpy()
    assert abs(on_device["auc"] - roc_auc_score(vl, 1 / (1 + np.exp(-logits.astype(np.float64))))) < 0.01
    z = logits.astype(np.float64)
    assert abs(on_device["loss"] - float((np.maximum(z, 0) - z * vl + np.log1p(np.exp(-np.abs(z)))).mean())) < 1e-4
    # a model no trainer holds is gathered into a flat buffer first: the same numbers
    fresh = make_model(0).cuda()
    fresh.load_state_dict({k: v.clone() for k, v in now.items()})
    assert evaluate_ctr(fresh, vu, vi, vl, batch_size=100) == on_device


@pytest.mark.gpu
def test_the_auc_is_that_of_the_stored_scores_and_a_nan_is_refused():
    from pmgt_amd import evaluate_ctr
    from pmgt_amd.dcn_train import DcnGrad, _flat_of
    from pmgt_amd.evaluation import roc_auc_score
    from pmgt_amd.metrics import ValidationMetrics
    from pmgt_amd.ncf_train import ng_sample
    _, valid = pair_lists()
    model = make_model(3).cuda()
    vu, vi, vl = ng_sample(valid, USERS, ITEMS, 5, 9)
    out = evaluate_ctr(model, vu, vi, vl, batch_size=64)
    dims, flat = _flat_of(model)
    logits = DcnGrad(*dims[:4], 1e-12, USERS, ITEMS, flat).forward(torch.from_numpy(vu).cuda(), torch.from_numpy(vi).cuda())
    vm = ValidationMetrics("cuda", len(vu))
    vm.update(logits, torch.from_numpy(vl).cuda())
    assert out["auc"] == vm.result()["val/auc"] == roc_auc_score(vm.labels(), vm.scores())      # one call of 480 pairs = eight batches: same bits
    with torch.no_grad():
        model.output_layer.bias.fill_(float("nan"))
    for metrics in ("device", "host"):
        with pytest.raises(ValueError, match="NaN"):
            evaluate_ctr(model, vu, vi, vl, metrics=metrics)
    with pytest.raises(ValueError, match="metrics"):
        evaluate_ctr(model, vu, vi, vl, metrics="gpu")
    with pytest.raises(ValueError, match="items"):
        evaluate_ctr(model, vu, vi + ITEMS, vl)


@pytest.mark.gpu
def test_early_stopping_and_refusals():
    from pmgt_amd import fit_dcn
    train, valid = pair_lists()
    # lr 0: nothing improves after the first epoch, patience 1 stops after the second
    history = fit_dcn(make_model(0).cuda(), train, valid, max_epochs=EPOCHS, early_criterion="loss", patience=1, **{**SETTINGS, "lr": 0.0})
    assert len(history) == 2 and [h["best"] for h in history] == [True, False] and history[0]["loss"] == history[1]["loss"]
    model = make_model(0).cuda()
    for kw, what in ((dict(early_criterion="n20"), "early_criterion"), (dict(batch_size=0), "batch_size"), (dict(batch_size=1 << 17), "batch_size")):
        with pytest.raises(ValueError, match=what):
            fit_dcn(model, train, valid, **{**dict(batch_size=64, max_epochs=1), **kw})
    with pytest.raises(ValueError, match="users"):
        fit_dcn(model, np.array([[USERS, 0]]), valid, batch_size=64, max_epochs=1)
    with pytest.raises(ValueError, match="dropout is not covered"):
        fit_dcn(DCN(USERS, ITEMS, 16, 1, 4, dropout=0.5).cuda(), train, valid, batch_size=64, max_epochs=1)


if __name__ == "__main__":
    runs = [torch_fit(s) for s in SEEDS]
    print("first " + "  ".join(f"{r[0]:.4f}" for r in runs))
    print("best  " + "  ".join(f"{max(r):.4f}" for r in runs))
    best = [max(r) for r in runs]
    print(f"bound = {min(best):.4f} - {max(best) - min(best):.4f} = {min(best) - (max(best) - min(best)):.4f}")
    for r in runs:
        print(" ".join(f"{a:.3f}" for a in r))
