"""fit_ncf(train_table=True) in the world and with the settings of tests/test_fit_ncf_gpu.py: the interaction list of
tests/golden/ranking_candidates.npz (40 users x 300 items, 519 pairs), a seeded item table, d = 64, head (16, 3, NeuMF-end), lr 1e-2,
num_ng 4, batches of 256, clipping at 5, 12 epochs -- with the table initialised from the seeded one and trained with the head.

THE BOUND, 0.35 x: the torch yardstick of the same procedure (tests/ncf_table_util.fit_table_yardstick) takes the mean training loss from
0.5874 to 0.1617 (0.275 x) with the table trained, the same to four digits in fp32 and fp64, and moves table entries by up to 0.81; with
the table frozen (tests/ncf_train_util.fit_yardstick) it reaches 0.368 x in fp32 and 0.378 x in fp64.  0.35 x lies between the two: a fit
whose table does not learn fails it, and the trained-table figure has a margin of 1.27 over its yardstick.  Measured on the MI355X (one run): 0.5874 -> 0.1466 (0.250 x), the table
moving by up to 0.854, n20 0.425 -> 0.977."""
import glob
import os

import numpy as np
import pytest
import torch

from pmgt_amd import fit_ncf, recommend
from pmgt_amd.evaluation import evaluate_ranking, rank_users
from pmgt_amd.metrics import RankingMetrics
from pmgt_amd.ncf_train import TABLE_KEY, head_state, table_layout
from tests.ncf_table_util import flat_buffer
from tests.test_fit_ncf_gpu import EPOCHS, SETTINGS, SHAPE, world

pytestmark = pytest.mark.gpu


def test_fit_trains_the_table_and_hands_the_best_one_back(tmp_path):
    g, model, w, table = world()
    initial = table.clone()
    valid = (g["users"], g["candidates"], g["labels"], g["counts"])
    history = fit_ncf(model, table, g["pairs"], valid, max_epochs=EPOCHS, early_criterion="n20", patience=EPOCHS, ckpt_dir=str(tmp_path),
                      train_table=True, **SETTINGS)
    assert len(history) == EPOCHS and all(np.isfinite(h[k]) for h in history for k in ("train_loss", "n10", "n20", "r10", "r20", "loss"))
    first, last = history[0]["train_loss"], history[-1]["train_loss"]
    moved = float((table - initial).abs().max())
    print(f"training loss {first:.4f} -> {last:.4f} ({last / first:.3f} x); the table moved by up to {moved:.3f}; n20 "
          + " ".join(f"{h['n20']:.3f}" for h in history))
    assert last <= 0.35 * first
    # the caller's table was overwritten in place with the best epoch's: the checkpoint's, and the one inside the trainer's buffer
    assert not torch.equal(table, initial) and bool(torch.isfinite(table).all())
    best = max((h for h in history if h["best"]), key=lambda h: h["epoch"])
    files = glob.glob(os.path.join(str(tmp_path), "*.ckpt"))
    assert [os.path.basename(f) for f in files] == [f"epoch={best['epoch']:02d}-n20={best['n20']:.4f}.ckpt"]
    ckpt = torch.load(files[0], weights_only=False)
    assert ckpt["epoch"] == best["epoch"] and torch.equal(ckpt[TABLE_KEY], table.cpu())
    now = head_state(model)
    assert sorted(ckpt["head"]) == sorted(now) == sorted(w) and all(torch.equal(now[k].cpu(), ckpt["head"][k]) for k in now)
    layout, count = table_layout(*SHAPE, int(g["num_user"]), int(g["num_item"]))
    flat = flat_buffer(model)
    off, shape = layout[TABLE_KEY]
    assert flat.numel() == count and torch.equal(flat[off:].view(shape), table)
    assert flat[off:].data_ptr() != table.data_ptr()         # (a copy back into the caller's tensor, not a re-pointing)
    # the public readers on the trained table
    res, per_user = evaluate_ranking(model, None, *valid, metrics="device", table=table, per_user=True)
    metrics = RankingMetrics(table.device, len(g["users"]), (10, 20))
    on_dev = [torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
              for a, dt in zip(valid, (np.int64, np.int64, np.float32, np.int32))]
    model.eval()
    rank_users(model, table, *on_dev, sink=metrics.update)
    assert res == metrics.result()
    host = evaluate_ranking(model, None, *valid, metrics="host", table=table)
    assert all(abs(host[k] - res[k]) <= 1e-9 for k in ("n10", "n20", "r10", "r20"))
    items, scores = recommend(model, None, g["users"][:8], k=10, table=table)
    assert items.shape == (8, 10) and np.isfinite(scores).all()
    with pytest.raises(ValueError, match="table"):
        evaluate_ranking(model, None, *valid, table=table[:-1])


def test_the_default_leaves_the_callers_table_alone():
    g, model, w, table = world()
    initial = table.clone()
    valid = (g["users"], g["candidates"], g["labels"], g["counts"])
    fit_ncf(model, table, g["pairs"], valid, max_epochs=1, **SETTINGS)
    assert torch.equal(table, initial)
