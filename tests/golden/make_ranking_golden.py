"""Generates tests/golden/ranking_*.npz: what the reference's ranking evaluation computes on small deterministic inputs.  Imports the
reference through `_ref_shim` (development container only, like make_golden.py); the fixtures hold inputs and recorded results.

  ranking_metrics_<U>x<C>.npz   tie-free fp32 logits [U, C] and labels with 1 .. > 20 positives per user; the reference's `predictions`
                                (torch.topk(k=100) on the CPU, pmgt/ncf/trainer.py:213-214), get_ndcg / get_recall at 10 and 20 over all
                                users and called per user (pmgt/metrics.py:16-37), BCEWithLogitsLoss per user (trainer.py:212)
  ranking_candidates.npz        an interaction list over 40 users x 300 items, the rows of NCFDataset(is_training=False, num_ng=50) read in
                                index order after np.random.seed(seed), and its `gt` (pmgt/ncf/datasets.py:65-83,115-128)

Run: python tests/golden/make_ranking_golden.py
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
from pmgt.ncf.datasets import NCFDataset  # noqa: E402  (reference)

TOPK = 100


def metrics_fixture(U, C, seed):
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((U, C)) * 3).astype(np.float32)
    n_pos = 1 + (np.arange(U) * 7) % 30 if U > 8 else np.array([1, 7, 20, 21, 40][:U])
    assert n_pos.min() == 1 and n_pos.max() > 20
    labels = np.zeros((U, C), dtype=np.float32)
    targets = []
    for u in range(U):
        where = np.sort(rng.choice(C, size=int(n_pos[u]), replace=False))
        labels[u, where] = 1.0
        targets.append(where)
    logits = (logits + np.float32(2.5) * labels).astype(np.float32)      # positives tend to rank high: every cut-off sees hits
    for row in logits:
        assert len(np.unique(row)) == C, "tied scores: torch.topk's order would be unspecified"
    mlb = MultiLabelBinarizer(sparse_output=True, classes=np.arange(C))
    gt = mlb.fit_transform(targets)
    items = torch.arange(C)                  # a candidate's item id is its index in the row
    loss_func = torch.nn.BCEWithLogitsLoss()
    predictions, losses = [], []
    for u in range(U):
        pred, label = torch.from_numpy(logits[u]), torch.from_numpy(labels[u])
        losses.append(loss_func(pred, label).item())
        _, indices = pred.topk(k=min(TOPK, C))
        predictions.append(items[indices].numpy())
    predictions = np.stack(predictions)
    out = dict(logits=logits, labels=labels, predictions=predictions.astype(np.int64), loss=np.asarray(losses, dtype=np.float64))
    for top in (10, 20):
        out[f"n{top}"] = np.float64(get_ndcg(predictions, gt, mlb, top=top))
        out[f"r{top}"] = np.float64(get_recall(predictions, gt, mlb, top=top))
        out[f"n{top}_user"] = np.array([get_ndcg(predictions[u:u + 1], gt[u:u + 1], mlb, top=top) for u in range(U)], dtype=np.float64)
        out[f"r{top}_user"] = np.array([get_recall(predictions[u:u + 1], gt[u:u + 1], mlb, top=top) for u in range(U)], dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, f"ranking_metrics_{U}x{C}.npz"), **out)
    print(f"ranking_metrics_{U}x{C}: n10 {out['n10']:.6f} n20 {out['n20']:.6f} r10 {out['r10']:.6f} r20 {out['r20']:.6f}")


def candidates_fixture(num_user=40, num_item=300, num_ng=50, seed=11, long_user=7, absent_user=13):
    rng = np.random.default_rng(3)
    pairs = []
    for u in range(num_user):
        if u == absent_user:
            continue                          # a user without interactions has no row
        n = 60 if u == long_user else int(rng.integers(1, 25))      # the long user: n_pos >= num_ng, no negatives
        pairs += [(u, int(i)) for i in rng.choice(num_item, size=n, replace=False)]
    # Users interleaved, every user's items in ascending order.  The reference reads a user's positives as `mat[u].indices` of
    # dok_matrix.tocsr(): the scipy of its time sorts them (coo -> csr sums duplicates), a current one keeps insertion order.  On this list
    # both give ascending positives, so the fixture does not depend on the scipy that wrote it; that ranking_candidates sorts is tested
    # on a shuffled copy of the list.
    pairs.sort(key=lambda p: (p[1], p[0]))
    ds = NCFDataset(pairs, num_user, num_item, num_ng=num_ng, is_training=False)
    np.random.seed(seed)
    rows = [ds[idx] for idx in range(len(ds))]
    c_max = max(len(r[1]) for r in rows)
    assert c_max == 60 and len(rows) == num_user - 1
    users = np.array([r[0][0] for r in rows], dtype=np.int64)
    counts = np.array([len(r[1]) for r in rows], dtype=np.int32)
    candidates = np.zeros((len(rows), c_max), dtype=np.int64)
    labels = np.zeros((len(rows), c_max), dtype=np.float32)
    for j, ((_, items), lab) in enumerate(rows):
        candidates[j, :len(items)] = items
        labels[j, :len(lab)] = lab
    np.savez_compressed(os.path.join(HERE, "ranking_candidates.npz"), pairs=np.asarray(pairs, dtype=np.int64), num_user=num_user,
                        num_item=num_item, num_ng=num_ng, seed=seed, long_user=long_user, users=users, candidates=candidates, labels=labels,
                        counts=counts, gt=np.asarray(ds.gt.todense()).astype(np.uint8))
    print(f"ranking_candidates: {len(rows)} users, C_max {c_max}, counts {counts.min()} .. {counts.max()}")


if __name__ == "__main__":
    metrics_fixture(64, 128, seed=1)
    metrics_fixture(5, 1000, seed=2)
    candidates_fixture()
