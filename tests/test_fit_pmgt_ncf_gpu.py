"""fit_pmgt_ncf: fine-tuning a PMGT_NCF, encoder and head, over epochs of sampled pairs with one sampled context per pair, ranking validation
with the CURRENT encoder, early stopping and the best encoder AND head restored.

The data: a synthetic graph of 48 nodes, 16 users; a user interacts with items of ONE half of the catalogue only (even users the lower
half, odd users the upper), and the two halves differ in the mean of their features, so the rule can be learnt through the encoder as well
as through the GMF rows.  Encoder hidden 64, 2 layers, 4 heads, S 16, fp32; head (16, 3, NeuMF-end); batch 32, 4 epochs, lr 1e-3.
The autograd path (PMGT_NCF.forward + backward, the encoder stepped by get_optimizer's AdamW over the engine's buffers -- which is all that
optimizer can hold -- and the head by torch.optim.AdamW) runs on the same finetune_batches and must show a decreasing loss too."""
import types

import numpy as np
import pytest
import torch

from pmgt_amd import finetune
from pmgt_amd.finetune import finetune_batches, fit_pmgt_ncf

pytestmark = pytest.mark.gpu

N_ITEMS, N_USERS, S, BATCH, EPOCHS, LR, NUM_NG = 48, 16, 16, 32, 4, 1e-3, 2
METRICS = ("n10", "n20", "r10", "r20", "loss")


def build():
    from pmgt_amd.configuration_pmgt import PMGTConfig
    from pmgt_amd.datasets import MCNSampler, ranking_candidates
    from pmgt_amd.graph import synthetic_graph
    from pmgt_amd.models import synthetic_features
    from pmgt_amd.pmgt_ncf import PMGT_NCF
    torch.manual_seed(0)
    cfg = PMGTConfig(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=64, feat_hidden_sizes=(32, 16),
                     hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    model = PMGT_NCF(user_num=N_USERS, item_num=N_ITEMS, factor_num=16, num_layers=3, model="NeuMF-end", config=cfg, dtype="fp32")
    feats = synthetic_features(N_ITEMS, (32, 16), seed=1)
    for f in feats:
        f[2 + N_ITEMS // 2:, : f.shape[1] // 2] += 1.5       # the upper half of the catalogue stands apart
    model.set_features(feats)
    sampler = MCNSampler(synthetic_graph(N_ITEMS, 200, seed=2), max_ctx_neigh=S - 1)
    rng = np.random.default_rng(3)
    train, valid = [], []
    for u in range(N_USERS):
        mine = (u % 2) * (N_ITEMS // 2) + rng.choice(N_ITEMS // 2, size=10, replace=False)
        train += [(u, int(i)) for i in mine[:8]]
        valid += [(u, int(i)) for i in mine[8:]]
    return model, sampler, np.asarray(train), ranking_candidates(valid, N_USERS, N_ITEMS, 20, seed=4)


def tensors_of(model):
    """The model's bert.* and head tensors (what the best file holds), cloned"""
    from pmgt_amd.ncf_head import HEAD_PREFIXES
    return {k: v.detach().clone() for k, v in model.state_dict().items() if k.startswith(("bert.",) + HEAD_PREFIXES)}


def test_fit_history_best_file_and_restored_model(tmp_path):
    from pmgt_amd.trainer import evaluate_ranking
    model, sampler, train, valid = build()
    model.train()
    untrained = evaluate_ranking(model, sampler, *valid, metrics="device")
    per_epoch = []
    history = fit_pmgt_ncf(model, sampler, train, valid, BATCH, EPOCHS, num_ng=NUM_NG, seed=0, lr=LR, ckpt_dir=str(tmp_path), patience=10,
                           log=lambda row: per_epoch.append(tensors_of(model)))
    assert model.training                                    # the mode the caller had
    assert [h["epoch"] for h in history] == list(range(EPOCHS)) and all(set(h) == {"epoch", "train_loss", "best", *METRICS} for h in history)
    print("trainer: " + ", ".join(f"epoch {h['epoch']} loss {h['train_loss']:.4f} n20 {h['n20']:.4f}" for h in history))
    assert all(np.isfinite(h["train_loss"]) for h in history) and history[-1]["train_loss"] < history[0]["train_loss"]
    assert history[0]["best"] and history[0]["n20"] != untrained["n20"]      # validation saw the trained encoder and head, not the initial ones
    best = max(range(EPOCHS), key=lambda e: (history[e]["n20"], -e))          # (strict improvement: the first of equal values)
    assert [h["best"] for h in history] == [all(history[e]["n20"] > history[j]["n20"] for j in range(e)) for e in range(EPOCHS)]
    files = sorted(p.name for p in tmp_path.iterdir())
    assert files == [f"epoch={best:02d}-n20={history[best]['n20']:.4f}.ckpt"]
    ckpt = torch.load(str(tmp_path / files[0]), map_location="cpu")
    assert ckpt["epoch"] == best and ckpt["metrics"] == history[best]
    now = tensors_of(model)
    saved = dict(ckpt["bert"], **ckpt["head"])
    assert set(saved) == set(now) and any(k.startswith("bert.encoder") for k in saved) and "gmf_item_embeddings.weight" in saved
    for k, v in now.items():
        assert torch.equal(v.cpu(), saved[k]), k
        assert torch.equal(v, per_epoch[best][k]), k
    # the restored model IS the best epoch's: the same validation again gives that epoch's row (and so validation ran on the current encoder)
    again = evaluate_ranking(model, sampler, *valid, metrics="device")
    assert all(again[k] == history[best][k] for k in METRICS), (again, history[best])
    # the head is the model's own parameters: no copy to go stale
    assert not torch.equal(per_epoch[0]["bert.encoder.layer.0.output.dense.weight"], per_epoch[-1]["bert.encoder.layer.0.output.dense.weight"])


def test_a_worsening_monitor_stops_early_and_the_best_epoch_comes_back(monkeypatch, tmp_path):
    model, sampler, train, valid = build()
    real = finetune.ranking_validator

    def worsening(*args, **kw):
        validate = real(*args, **kw)
        return lambda epoch: dict(validate(epoch), n20=1.0 / (1 + epoch))
    monkeypatch.setattr(finetune, "ranking_validator", worsening)
    model.eval()
    per_epoch = []
    history = fit_pmgt_ncf(model, sampler, train, valid, BATCH, EPOCHS, num_ng=NUM_NG, seed=0, lr=LR, ckpt_dir=str(tmp_path), patience=2,
                           log=lambda row: per_epoch.append(tensors_of(model)))
    assert not model.training
    assert [h["best"] for h in history] == [True, False, False] and len(per_epoch) == 3      # stopped after two epochs without improvement
    now = tensors_of(model)
    ckpt = torch.load(str(tmp_path / "epoch=00-n20=1.0000.ckpt"), map_location="cpu")
    moved = 0
    for k, v in now.items():
        assert torch.equal(v, per_epoch[0][k]) and torch.equal(v.cpu(), dict(ckpt["bert"], **ckpt["head"])[k]), k
        moved += int(not torch.equal(v, per_epoch[-1][k]))
    assert moved >= len(now) - 2                             # (position_ids / role_ids are buffers: they never move)


def test_the_autograd_path_learns_on_the_same_batches():
    from pmgt_amd.optimizers import get_optimizer
    model, sampler, train, _ = build()
    model.train()
    enc_opt = get_optimizer(types.SimpleNamespace(model=model.bert, decay=0.0, lr=LR, optim="adamw", gradient_max_norm=5.0))
    head = [p for k, p in model.named_parameters() if p.requires_grad and not k.startswith("bert.")]
    head_opt = torch.optim.AdamW(head, lr=LR, weight_decay=0.0)
    means = []
    for epoch in range(EPOCHS):
        losses = []
        for users, items, labels, node_ids, mask in finetune_batches(train, sampler, N_USERS, N_ITEMS, BATCH, NUM_NG, 0, epoch):
            assert np.array_equal(node_ids[:, 0], items + 2)
            logits = model(torch.from_numpy(users), {"node_ids": torch.from_numpy(node_ids), "attention_mask": torch.from_numpy(mask)})
            loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, torch.from_numpy(labels).cuda())
            enc_opt.zero_grad(), head_opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(head, 5.0)
            enc_opt.step(), head_opt.step()
            losses.append(loss.detach())
        means.append(float(torch.stack(losses).mean()))
    print("autograd: " + ", ".join(f"epoch {e} loss {m:.4f}" for e, m in enumerate(means)))
    assert means[-1] < means[0]
