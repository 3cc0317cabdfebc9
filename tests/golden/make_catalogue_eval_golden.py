"""Generates tests/golden/catalogue_eval_48x300.npz: what the reference's metrics give on whole-catalogue lists.  Imports the reference
through `_ref_shim` (development container only, like make_ranking_golden.py); the fixture holds inputs and recorded results.

  scores        fp32 [48, 300], distinct within every row (torch.topk's order is then defined)
  excl_indptr, excl_items      exclusion lists of 0 .. 40 items per user
  held_indptr, held_items      held-out lists of 1 .. > 20 items per user, disjoint from the exclusions
  predictions   the reference's `predictions` (pmgt/ncf/trainer.py:213-214): torch.topk(100) of each row with the excluded entries at -inf
  n10, n20, r10, r20 and *_user    get_ndcg / get_recall (pmgt/metrics.py:16-37) over all users and called per user

Run: python tests/golden/make_catalogue_eval_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_shim  # noqa: E402

_ref_shim.install()

from sklearn.preprocessing import MultiLabelBinarizer  # noqa: E402

from pmgt.metrics import get_ndcg, get_recall  # noqa: E402  (reference)

TOPK = 100


def fixture(U=48, n_items=300, seed=5):
    rng = np.random.default_rng(seed)
    scores = (rng.standard_normal((U, n_items)) * 3).astype(np.float32)
    n_excl = (np.arange(U) * 11) % 41                        # 0 .. 40
    n_held = 1 + (np.arange(U) * 7) % 30                     # 1 .. 30
    assert n_excl.min() == 0 and n_excl.max() == 40 and n_held.min() == 1 and n_held.max() > 20
    excl, held = [], []
    for u in range(U):
        drawn = rng.choice(n_items, size=int(n_excl[u] + n_held[u]), replace=False)
        excl.append(np.sort(drawn[: n_excl[u]]))
        held.append(np.sort(drawn[n_excl[u]:]))
        scores[u, held[u]] += np.float32(2.5)                 # held-out items tend to rank high: every cut-off sees hits
    masked = scores.copy()
    for u in range(U):
        masked[u, excl[u]] = -np.inf
        eligible = np.setdiff1d(np.arange(n_items), excl[u])
        assert len(np.unique(scores[u, eligible])) == len(eligible), "tied scores: torch.topk's order would be unspecified"
        assert n_items - len(excl[u]) >= TOPK
    mlb = MultiLabelBinarizer(sparse_output=True, classes=np.arange(n_items))
    gt = mlb.fit_transform(held)
    predictions = np.stack([torch.from_numpy(masked[u]).topk(k=TOPK)[1].numpy() for u in range(U)]).astype(np.int64)
    out = dict(scores=scores, predictions=predictions,
               excl_indptr=np.concatenate([[0], np.cumsum([len(e) for e in excl])]).astype(np.int64),
               excl_items=np.concatenate(excl).astype(np.int32),
               held_indptr=np.concatenate([[0], np.cumsum([len(h) for h in held])]).astype(np.int64),
               held_items=np.concatenate(held).astype(np.int32))
    for top in (10, 20):
        out[f"n{top}"] = np.float64(get_ndcg(predictions, gt, mlb, top=top))
        out[f"r{top}"] = np.float64(get_recall(predictions, gt, mlb, top=top))
        out[f"n{top}_user"] = np.array([get_ndcg(predictions[u:u + 1], gt[u:u + 1], mlb, top=top) for u in range(U)], dtype=np.float64)
        out[f"r{top}_user"] = np.array([get_recall(predictions[u:u + 1], gt[u:u + 1], mlb, top=top) for u in range(U)], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, f"catalogue_eval_{U}x{n_items}.npz"), **out)
    print(f"catalogue_eval_{U}x{n_items}: n10 {out['n10']:.6f} n20 {out['n20']:.6f} r10 {out['r10']:.6f} r20 {out['r20']:.6f}")


if __name__ == "__main__":
    fixture()
