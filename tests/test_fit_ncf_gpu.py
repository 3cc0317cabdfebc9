"""fit_ncf on the interaction list of tests/golden/ranking_candidates.npz (40 users x 300 items, 519 pairs) over a seeded random item table:
d = 64, head (16, 3, NeuMF-end), lr 1e-2, num_ng 4, batches of 256 (eleven steps an epoch, the last one short), clipping at 5.

THE EPOCH COUNT, 12, was chosen on the CPU with the torch yardstick of the same procedure (tests/ncf_train_util.fit_yardstick: ng_sample,
epoch_order, the head's formula in fp32 torch, autograd, clip_grad_norm_, AdamW): the smallest count at which its last epoch's mean training
loss is at most 0.4 x its first epoch's.  Its figures: epoch 1 0.5878, epoch 11 0.2656 (0.452 x), epoch 12 0.2162 (0.368 x); the same
procedure in fp64: 0.5878, 0.2683, 0.2225.  The device fit must reach 0.5 x."""
import glob
import os

import numpy as np
import pytest
import torch

from pmgt_amd import fit_ncf
from pmgt_amd.ncf_train import head_state
from tests.ncf_train_util import make_model

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ranking_candidates.npz")
SHAPE, EPOCHS, SEED = (16, 3, "NeuMF-end"), 12, 77
SETTINGS = dict(batch_size=256, num_ng=4, seed=0, lr=1e-2, max_grad_norm=5.0)


def world():
    g = np.load(GOLD)
    model, w, table = make_model(*SHAPE, int(g["num_user"]), int(g["num_item"]), SEED)
    return g, model, w, torch.from_numpy(table).cuda()


def test_fit_learns_validates_and_keeps_the_best_head(tmp_path):
    g, model, w, table = world()
    valid = (g["users"], g["candidates"], g["labels"], g["counts"])
    seen = []
    history = fit_ncf(model, table, g["pairs"], valid, max_epochs=EPOCHS, early_criterion="n20", patience=EPOCHS, ckpt_dir=str(tmp_path),
                      log=seen.append, **SETTINGS)
    assert len(history) == EPOCHS and seen == history and [h["epoch"] for h in history] == list(range(EPOCHS))
    for h in history:
        assert all(np.isfinite(h[k]) for k in ("train_loss", "n10", "n20", "r10", "r20", "loss"))
        assert 0 <= h["n10"] <= 1 and 0 <= h["n20"] <= 1 and 0 <= h["r10"] <= h["r20"] <= 1 and h["loss"] > 0
    first, last = history[0]["train_loss"], history[-1]["train_loss"]
    print(f"training loss {first:.4f} -> {last:.4f} ({last / first:.3f} x); n20 " + " ".join(f"{h['n20']:.3f}" for h in history))
    assert last <= 0.5 * first
    # the best epoch by n20: strictly better than everything before it; its head is in the model and in the one checkpoint file
    best = max((h for h in history if h["best"]), key=lambda h: h["epoch"])
    assert best["n20"] == max(h["n20"] for h in history) and all(h["n20"] < best["n20"] for h in history[:best["epoch"]])
    files = glob.glob(os.path.join(str(tmp_path), "*.ckpt"))
    assert [os.path.basename(f) for f in files] == [f"epoch={best['epoch']:02d}-n20={best['n20']:.4f}.ckpt"]
    ckpt = torch.load(files[0], weights_only=False)
    now = head_state(model)
    assert ckpt["epoch"] == best["epoch"] and sorted(ckpt["head"]) == sorted(now) == sorted(w)
    assert all(torch.equal(now[k].cpu(), ckpt["head"][k]) for k in now)
    assert any(not np.array_equal(now[k].cpu().numpy(), w[k]) for k in w)
    if best["epoch"] != EPOCHS - 1:
        print(f"the best epoch is {best['epoch']}, not the last: the restored head differs from the last step's")


def test_a_criterion_that_cannot_improve_stops_after_the_second_epoch():
    g, model, w, table = world()
    valid = (g["users"], g["candidates"], np.zeros_like(g["labels"]), g["counts"])      # no positive anywhere: n20 = 0 every epoch
    history = fit_ncf(model, table, g["pairs"], valid, max_epochs=EPOCHS, early_criterion="n20", patience=1, **SETTINGS)
    assert len(history) == 2 and [h["best"] for h in history] == [True, False]
    assert all(h["n20"] == 0 and h["r20"] == 0 for h in history) and history[1]["train_loss"] < history[0]["train_loss"]


def test_fit_refusals():
    g, model, w, table = world()
    valid = (g["users"], g["candidates"], g["labels"], g["counts"])
    for kw, what in ((dict(early_criterion="auc"), "early_criterion"), (dict(batch_size=0), "batch_size"), (dict(batch_size=1 << 17), "batch_size")):
        with pytest.raises(ValueError, match=what):
            fit_ncf(model, table, g["pairs"], valid, **{**dict(batch_size=256, max_epochs=1), **kw})
    with pytest.raises(ValueError, match="users"):
        fit_ncf(model, table, np.array([[40, 0]]), valid, batch_size=256, max_epochs=1)
    with pytest.raises(ValueError, match="validation"):
        fit_ncf(model, table, g["pairs"], (g["users"], g["candidates"] + 300, g["labels"], g["counts"]), batch_size=256, max_epochs=1)
