"""Generates tests/golden/ncf_ng_sample.npz: what the reference's training-mode negative sampling draws on a small interaction list.
Imports the reference through `_ref_shim` (development container only, like make_ranking_golden.py); the fixture holds inputs and recorded
results.

  ncf_ng_sample.npz   an interaction list over 40 users x 300 items in which one user holds most items (their negatives are redrawn many
                      times), and for num_ng in (1, 4) the `features` and `labels` of NCFDataset(pairs, ..., num_ng, is_training=True) after
                      np.random.seed(seed); ng_sample() (pmgt/ncf/datasets.py:85-101)

Run: python tests/golden/make_ncf_train_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_shim  # noqa: E402

_ref_shim.install()

from pmgt.ncf.datasets import NCFDataset  # noqa: E402  (reference)


def ng_sample_fixture(num_user=40, num_item=300, greedy_user=5, seeds=(17, 18)):
    rng = np.random.default_rng(5)
    pairs = []
    for u in range(num_user):
        n = 270 if u == greedy_user else int(rng.integers(1, 25))      # the greedy user: nine draws in ten are rejected
        pairs += [(u, int(i)) for i in rng.choice(num_item, size=n, replace=False)]
    pairs = [pairs[j] for j in rng.permutation(len(pairs))]           # users interleaved
    out = dict(pairs=np.asarray(pairs, dtype=np.int64), num_user=num_user, num_item=num_item, greedy_user=greedy_user)
    for num_ng, seed in zip((1, 4), seeds):
        ds = NCFDataset(pairs, num_user, num_item, num_ng=num_ng, is_training=True)
        np.random.seed(seed)
        ds.ng_sample()
        feats = np.asarray(ds.features, dtype=np.int64)
        assert feats.shape == (len(pairs) * (1 + num_ng), 2) and len(ds.labels) == len(feats)
        out[f"seed_ng{num_ng}"] = seed
        out[f"users_ng{num_ng}"] = feats[:, 0]
        out[f"items_ng{num_ng}"] = feats[:, 1]
        out[f"labels_ng{num_ng}"] = np.asarray(ds.labels, dtype=np.float32)
        print(f"ncf_ng_sample: num_ng {num_ng}: {len(feats)} rows")
    np.savez_compressed(os.path.join(HERE, "ncf_ng_sample.npz"), **out)


if __name__ == "__main__":
    ng_sample_fixture()
