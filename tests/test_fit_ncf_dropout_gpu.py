"""fit_ncf(dropout_seed=...) in the world and with the settings of tests/test_fit_ncf_gpu.py (40 users x 300 items, 519 pairs, head
(16, 3, NeuMF-end) over a frozen seeded table, lr 1e-2, num_ng 4, batches of 256, clipping at 5, 12 epochs), dropout = emb_dropout = 0.2.

THE CONVERGENCE BOUND is on final / initial validation loss (the "loss" of the last epoch's row over that of epoch 0's: the mean over the
validation users of the mean BCE-with-logits over their candidates, in eval mode).  It was derived on the CPU with torch_dropout_fit below:
the same procedure -- ng_sample, epoch_order, the head's formula in fp32 torch, autograd, clip_grad_norm_, AdamW -- with torch's own
dropout (torch.nn.functional.dropout in training mode) in place of the device's masks, over the torch seeds 0 .. 5.  The device's mask stream
is one more draw of the same distribution, so it is held to the worst seed's ratio plus the spread (max - min) of the seeds:
    seed     0       1       2       3       4       5
    initial  0.5899  0.5888  0.5881  0.5926  0.5817  0.5928
    final    0.4282  0.4216  0.4282  0.4240  0.4395  0.4326
    ratio    0.7258  0.7160  0.7282  0.7155  0.7555  0.7297
    bound = max + (max - min) = 0.7555 + 0.0400 = 0.7955
(python -m tests.test_fit_ncf_dropout_gpu prints them again; no GPU is needed for that.)  Measured on the MI355X (one run): the device fit went 0.5874 -> 0.4334, ratio 0.7378; n20 0.402 -> 0.773."""

import numpy as np
import pytest
import torch

from pmgt_amd import fit_ncf
from tests.test_fit_ncf_gpu import EPOCHS, GOLD, SEED, SETTINGS, SHAPE

P = 0.2
DROPOUT_SEED = 5
SEEDS = (0, 1, 2, 3, 4, 5)
SEED_RATIOS = (0.7258, 0.7160, 0.7282, 0.7155, 0.7555, 0.7297)      # torch seeds 0 .. 5: 0.59 -> 0.43 each; without dropout 0.5841 -> 0.2046
RATIO_BOUND = max(SEED_RATIOS) + (max(SEED_RATIOS) - min(SEED_RATIOS))


def torch_dropout_fit(torch_seed, p=P):
    """fit_ncf's loop on the CPU in fp32 torch with torch's own dropout stream -> the validation loss after every epoch."""
    import torch.nn.functional as F
    from pmgt_amd.fit_loop import epoch_order
    from pmgt_amd.ncf_train import ng_sample
    from tests.test_recommend_cpu import random_head
    g = np.load(GOLD)
    num_user, num_item = int(g["num_user"]), int(g["num_item"])
    w, table = random_head(*SHAPE, num_user, num_item, SEED)
    prm = {k: torch.tensor(v, requires_grad=True) for k, v in w.items()}
    table = torch.from_numpy(table)
    opt = torch.optim.AdamW([{"params": [v for k, v in prm.items() if not k.endswith(".bias")], "weight_decay": 0.0},
                             {"params": [v for k, v in prm.items() if k.endswith(".bias")], "weight_decay": 0.0}], lr=SETTINGS["lr"])

    def logits(u, it, training):
        x = F.dropout(torch.cat([prm["mlp_user_embeddings.weight"][u], table[it]], dim=-1), p, training)
        for i in range(SHAPE[1]):
            x = torch.relu(F.dropout(x @ prm[f"mlp_layers.{i}.linear.weight"].T + prm[f"mlp_layers.{i}.linear.bias"], p, training))
        gmf = F.dropout(prm["gmf_user_embeddings.weight"][u] * prm["gmf_item_embeddings.weight"][it], p, training)
        return (torch.cat([gmf, x], dim=-1) @ prm["predict_layer.weight"].T + prm["predict_layer.bias"]).view(-1)

    vu, vc, vl, cnt = (torch.from_numpy(g[k]) for k in ("users", "candidates", "labels", "counts"))
    live = torch.arange(vc.shape[1])[None, :] < cnt[:, None]
    torch.manual_seed(torch_seed)
    out = []
    for epoch in range(EPOCHS):
        users, items, labels = ng_sample(g["pairs"], num_user, num_item, SETTINGS["num_ng"], SETTINGS["seed"] + epoch)
        order = epoch_order(len(users), SETTINGS["seed"], epoch)
        users, items, labels = (torch.from_numpy(a[order]) for a in (users, items, labels))
        for lo in range(0, len(order), SETTINGS["batch_size"]):
            hi = lo + SETTINGS["batch_size"]
            opt.zero_grad(set_to_none=True)
            F.binary_cross_entropy_with_logits(logits(users[lo:hi], items[lo:hi], True), labels[lo:hi]).backward()
            torch.nn.utils.clip_grad_norm_(list(prm.values()), SETTINGS["max_grad_norm"])
            opt.step()
        with torch.no_grad():
            z = logits(vu[:, None].expand_as(vc).reshape(-1), vc.reshape(-1), False).view(vc.shape)
            per = F.binary_cross_entropy_with_logits(z, (vl != 0).float(), reduction="none")
            out.append(float(((per * live).sum(1) / cnt).mean()))
    return out


def world(p=P):
    from tests.ncf_train_util import make_model
    g = np.load(GOLD)
    model, w, table = make_model(*SHAPE, int(g["num_user"]), int(g["num_item"]), SEED)
    model.emb_dropout.p = p
    for layer in model.mlp_layers:
        layer.dropout.p = p
    return g, model, torch.from_numpy(table).cuda()


def fit(p=P, dropout_seed=DROPOUT_SEED):
    g, model, table = world(p)
    valid = (g["users"], g["candidates"], g["labels"], g["counts"])
    history = fit_ncf(model, table, g["pairs"], valid, max_epochs=EPOCHS, early_criterion="n20", patience=EPOCHS, dropout_seed=dropout_seed,
                      **SETTINGS)
    return history, model


@pytest.mark.gpu
def test_the_fit_with_dropout_is_a_function_of_the_seed_differs_from_the_fit_without_and_converges():
    first, model = fit()
    again, _ = fit()
    assert first == again and len(first) == EPOCHS           # one seed, one history: every loss and metric of every epoch
    plain, _ = fit(p=0.0, dropout_seed=None)
    other, _ = fit(dropout_seed=DROPOUT_SEED + 1)
    assert [h["train_loss"] for h in first] != [h["train_loss"] for h in plain] and first[0]["loss"] != plain[0]["loss"]
    assert [h["train_loss"] for h in first] != [h["train_loss"] for h in other]
    # training mode costs training loss: the masked head fits the same batches worse than the head without dropout
    assert first[-1]["train_loss"] > plain[-1]["train_loss"]
    for h in first:
        assert all(np.isfinite(h[k]) for k in ("train_loss", "n10", "n20", "r10", "r20", "loss"))
    ratio = first[-1]["loss"] / first[0]["loss"]
    print(f"validation loss {first[0]['loss']:.4f} -> {first[-1]['loss']:.4f} ({ratio:.4f} x, bound {RATIO_BOUND:.4f}); without dropout "
          f"{plain[0]['loss']:.4f} -> {plain[-1]['loss']:.4f}; n20 " + " ".join(f"{h['n20']:.3f}" for h in first))
    assert max(h["n20"] for h in first[1:]) > first[0]["n20"]      # validation n20 improves over epoch 0
    assert ratio <= RATIO_BOUND, (ratio, RATIO_BOUND)


@pytest.mark.gpu
def test_a_model_with_dropout_and_no_seed_is_refused_by_the_fit():
    g, model, table = world()
    valid = (g["users"], g["candidates"], g["labels"], g["counts"])
    with pytest.raises(ValueError, match="dropout.*dropout_seed"):
        fit_ncf(model, table, g["pairs"], valid, max_epochs=1, **SETTINGS)


if __name__ == "__main__":
    rows = [torch_dropout_fit(s) for s in SEEDS]
    for s, r in zip(SEEDS, rows):
        print(f"torch seed {s}: validation loss " + " ".join(f"{x:.4f}" for x in r) + f"; final / initial {r[-1] / r[0]:.4f}")
    rt = [r[-1] / r[0] for r in rows]
    print(f"worst {max(rt):.4f}, spread {max(rt) - min(rt):.4f}, bound {max(rt) + max(rt) - min(rt):.4f}")
