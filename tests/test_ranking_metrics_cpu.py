"""The host side of the top-N ranking evaluation, no GPU: ranking_metrics_host against what the reference computes per user
(tests/golden/ranking_metrics_*.npz, written by tests/golden/make_ranking_golden.py), ranking_candidates against the reference's test-mode
dataset (ranking_candidates.npz), the tie rule, and the exported entries."""
import os
import subprocess

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
METRIC_FIXTURES = ["ranking_metrics_64x128", "ranking_metrics_5x1000"]


def load(name):
    return np.load(os.path.join(GOLDEN, name + ".npz"))


@pytest.mark.parametrize("name", METRIC_FIXTURES)
def test_host_metrics_equal_the_reference_per_user(name):
    from pmgt_amd.evaluation import ranking_metrics_host, summarize_ranking
    g = load(name)
    logits, labels = g["logits"], g["labels"]
    U = len(logits)
    got = ranking_metrics_host(logits, labels, None, (10, 20))
    for k in (10, 20):
        assert np.array_equal(got["ndcg"][k], g[f"n{k}_user"]), k          # bit for bit: the host's table, ascending adds, one division
        assert np.array_equal(got["recall"][k], g[f"r{k}_user"]), k
    assert np.array_equal(got["order"][:, :g["predictions"].shape[1]], g["predictions"])      # torch.topk(k=100) on tie-free scores
    assert np.array_equal(got["n_pos"], (labels != 0).sum(axis=1))
    assert int(got["n_pos"].min()) == 1 and int(got["n_pos"].max()) > 20
    # the means: any summation order of U values in [0, 1] stays within U * 2^-52 of any other
    res = summarize_ranking(got, (10, 20))
    for key in ("n10", "n20", "r10", "r20"):
        print(f"{name} {key}: host {res[key]!r} reference {float(g[key])!r}")
        assert abs(res[key] - float(g[key])) <= U * 2.0 ** -52, key
    # per-user loss: the reference's BCEWithLogitsLoss is an fp32 mean of C non-negative terms
    C = logits.shape[1]
    rel = np.abs(got["loss"].astype(np.float64) - g["loss"]) / g["loss"]
    print(f"{name} loss: largest relative distance to BCEWithLogitsLoss {rel.max():.3e}")
    assert rel.max() <= (C + 8) * 2.0 ** -24


def test_discount_tables_are_the_references_for_every_top():
    """get_ndcg builds 1 / log2(arange(top) + 2) per call; the one table of max(ks) entries must hold the same numbers for every top."""
    from pmgt_amd.metrics import discount_tables
    disc, idcg = discount_tables(1024)
    for top in (1, 5, 7, 10, 20, 64, 100, 1024):
        log = 1.0 / np.log2(np.arange(top) + 2)
        assert np.array_equal(disc[:top], log) and np.array_equal(idcg[:top], log.cumsum()), top


def test_candidates_equal_the_reference_dataset():
    from pmgt_amd.datasets import ranking_candidates
    g = load("ranking_candidates")
    num_ng = int(g["num_ng"])
    users, cand, labels, counts = ranking_candidates(g["pairs"], int(g["num_user"]), int(g["num_item"]), num_ng, int(g["seed"]))
    assert users.dtype == np.int64 and cand.dtype == np.int64 and labels.dtype == np.float32 and counts.dtype == np.int32
    assert np.array_equal(users, g["users"]) and np.array_equal(counts, g["counts"])
    assert np.array_equal(cand, g["candidates"]) and np.array_equal(labels, g["labels"])
    # the over-long user: all its positives, no negative, and it sets C_max
    row = int(np.flatnonzero(users == int(g["long_user"]))[0])
    n_pos = int(g["gt"][row].sum())
    assert n_pos >= num_ng and cand.shape[1] == n_pos == counts[row] and bool((labels[row] == 1).all())
    assert bool((counts[np.arange(len(users)) != row] == num_ng).all())
    # a user's positives are the reference's gt row, ascending
    for r in range(len(users)):
        pos = cand[r, :counts[r]][labels[r, :counts[r]] != 0]
        assert np.array_equal(pos, np.flatnonzero(g["gt"][r])), r
        neg = cand[r, :counts[r]][labels[r, :counts[r]] == 0]
        assert not g["gt"][r][neg].any(), r
    # the order of the interaction list does not matter (the fixture's list has every user's items ascending; the reference's own order of
    # a user's positives depends on its scipy: sorted in the one of its time, and that is the rule here), nor does a repeated pair
    shuffled = g["pairs"][np.random.default_rng(0).permutation(len(g["pairs"]))]
    shuffled = np.concatenate([shuffled, shuffled[:5]])
    assert all(np.array_equal(a, b) for a, b in zip(ranking_candidates(shuffled, int(g["num_user"]), int(g["num_item"]), num_ng, int(g["seed"])),
                                                    (users, cand, labels, counts)))
    # another seed draws other negatives, the same seed the same ones
    again = ranking_candidates(g["pairs"], int(g["num_user"]), int(g["num_item"]), num_ng, int(g["seed"]))
    other = ranking_candidates(g["pairs"], int(g["num_user"]), int(g["num_item"]), num_ng, int(g["seed"]) + 1)
    assert all(np.array_equal(a, b) for a, b in zip(again, (users, cand, labels, counts)))
    assert not np.array_equal(other[1], cand) and np.array_equal(other[3], counts)


def test_the_tie_rule_lower_index_first():
    from pmgt_amd.evaluation import ranking_metrics_host
    from pmgt_amd.metrics import discount_tables
    x = np.array([[1.0, 2.0, 1.0, 2.0, 0.5, 1.0],
                  [0.0, -0.0, 0.0, -0.0, 0.0, -0.0]], dtype=np.float32)
    y = np.array([[0, 0, 1, 1, 0, 1],
                  [0, 0, 0, 1, 0, 1]], dtype=np.float32)
    got = ranking_metrics_host(x, y, None, (1, 2, 4))
    assert got["order"].tolist() == [[1, 3, 0, 2, 5, 4], [0, 1, 2, 3, 4, 5]]       # equal scores (and the two zeros) keep their index order
    disc, idcg = discount_tables(4)
    # row 0: positives at ranks 1, 3, 4; row 1: at ranks 3, 5
    assert got["recall"][1].tolist() == [0.0, 0.0] and got["recall"][2].tolist() == [1 / 3, 0.0] and got["recall"][4].tolist() == [2 / 3, 0.5]
    assert got["ndcg"][2].tolist() == [disc[1] / idcg[1], 0.0]
    assert got["ndcg"][4].tolist() == [(disc[1] + disc[3]) / idcg[2], disc[3] / idcg[1]]
    # padding is never read: NaN behind the count changes nothing, a live NaN is flagged
    xp = np.concatenate([x, np.full((2, 2), np.nan, np.float32)], axis=1)
    yp = np.concatenate([y, np.ones((2, 2), np.float32)], axis=1)
    pad = ranking_metrics_host(xp, yp, np.array([6, 6]), (1, 2, 4))
    for k in (1, 2, 4):
        assert np.array_equal(pad["ndcg"][k], got["ndcg"][k]) and np.array_equal(pad["recall"][k], got["recall"][k])
    assert np.array_equal(pad["loss"], got["loss"]) and not pad["nan"].any() and pad["order"][:, 6:].tolist() == [[-1, -1], [-1, -1]]
    assert ranking_metrics_host(xp, yp, np.array([6, 7]), (1,))["nan"].tolist() == [False, True]


def test_summary_refuses_nan_and_empty_rows_and_bad_cutoffs():
    from pmgt_amd.evaluation import ranking_metrics_host, summarize_ranking
    x = np.array([[1.0, np.nan], [0.5, 0.25], [1.0, 2.0]], dtype=np.float32)
    y = np.array([[1, 0], [0, 0], [0, 1]], dtype=np.float32)
    with pytest.raises(ValueError, match="1 of 3 users have a NaN logit"):
        summarize_ranking(ranking_metrics_host(x, y, None, (1,)), (1,))
    x[0, 1] = 0.0
    with pytest.raises(ValueError, match="1 of 3 users have no positive candidate"):
        summarize_ranking(ranking_metrics_host(x, y, None, (1,)), (1,))
    for ks in ((), (0,), (5, 5), (20, 10), (1, 2, 3, 4, 5), (1025,)):
        with pytest.raises(ValueError):
            ranking_metrics_host(x, y, None, ks)


def test_library_exports_the_rank_entries_and_the_old_import_path_serves_the_new_names():
    from pmgt_amd import _build, _lib, evaluation, trainer
    out = subprocess.run(["nm", "-D", _build.hip_lib_path()], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pmgt_capi.h")).read()
    for sym in ("pmgt_rank_workspace_bytes", "pmgt_rank_reset", "pmgt_rank_append", "pmgt_rank_reduce"):
        assert sym in names and sym in _lib.HIP_SYMBOLS, sym
        decl = hdr[:hdr.index(sym + "(")]
        assert "pmgt/ncf/trainer.py:2" in decl[decl.rindex("/*"):], sym      # every entry cites the interface it replaces
    for name in ("evaluate_ranking", "ranking_metrics_host", "encode_catalogue", "rank_users"):
        assert getattr(trainer, name) is getattr(evaluation, name), name
