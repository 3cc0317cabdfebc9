"""The numpy side of recommending from a user's history: history_scores_host against a plain double loop, history_csr, and
recommend_from_history / evaluate_history(impl="host") on the planted table, with their refusals.  No GPU."""
import os
import re

import numpy as np
import pytest

from pmgt_amd import _build, _lib
from pmgt_amd.catalogue_eval import catalogue_metrics_host, heldout_csr, heldout_ranks_host
from pmgt_amd.history import evaluate_history, history_csr, history_scores_host, recommend_from_history, reduce_history
from pmgt_amd.recommend import topk_host
from pmgt_amd.similar import item_sim_host
from tests import item_sim_util as U

AGGS = ("mean", "max")


def planted_world():
    """8 users on planted_table(): user c has the items 5c, 5c + 2, 5c + 3 of cluster c; 5c + 1 and 5c + 4 are held out"""
    hist = np.array([(c, 5 * c + a) for c in range(8) for a in (0, 2, 3)], dtype=np.int64)
    held = np.array([(c, 5 * c + a) for c in range(8) for a in (1, 4)], dtype=np.int64)
    return U.planted_table(), hist, held


def random_histories(n_users, n_items, seed=3):
    """(user, item) pairs: user u has 1 + (u mod 7) distinct items, in no order"""
    rng = np.random.default_rng(seed)
    pairs = [(u, int(i)) for u in range(n_users) for i in rng.choice(n_items, size=1 + u % 7, replace=False)]
    return np.array(pairs, dtype=np.int64)[rng.permutation(len(pairs))]


@pytest.mark.parametrize("agg", AGGS)
def test_history_scores_host_is_the_plain_double_loop(agg):
    f32 = np.float32
    t = U.integer_table(33, 60)
    pairs = random_histories(12, 60)
    users = np.array([3, 0, 11, 3, 6], dtype=np.int64)
    got = history_scores_host(t, pairs, users, agg, "dot")
    assert got.dtype == np.float32 and got.shape == (5, 60)
    want = np.empty((5, 60), dtype=f32)
    for r, u in enumerate(users):
        mine = sorted({int(i) for v, i in pairs if v == u})
        for j in range(60):
            acc = None
            for i in mine:
                s = f32(0)
                for k in range(33):
                    s = f32(s + t[i, k] * t[j, k])
                acc = s if acc is None else (f32(acc + s) if agg == "mean" else max(acc, s))
            want[r, j] = f32(acc / f32(len(mine))) if agg == "mean" else acc + f32(0)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the composition it is stated as: item_sim_host's rows of the history items, then the reduction
    indptr, items = history_csr(pairs, 60)
    for metric in ("cosine", "dot"):
        full = history_scores_host(t, pairs, users, agg, metric)
        for r, u in enumerate(users):
            rows = item_sim_host(t, items[indptr[u]: indptr[u + 1]], metric)
            assert np.array_equal(full[r], reduce_history(rows, agg))
    assert history_scores_host(t, pairs, users, agg, "cosine", dtype=np.float64).dtype == np.float64


def test_the_reduction_as_defined():
    f32 = np.float32
    rows = np.array([[1e8, -0.0, 1.0, np.nan, 3.0], [1.0, -0.0, -2.0, 5.0, np.nan], [-1e8, 0.0, 1.5, 1.0, 1.0]], dtype=f32)
    mean = reduce_history(rows, "mean")
    assert mean[0] == f32(f32(f32(1e8) + f32(1)) + f32(-1e8)) / f32(3) and mean[0] == 0.0      # in order: the 1 is rounded away
    assert np.isnan(mean[3]) and np.isnan(mean[4]) and mean[2] == f32(f32(0.5) / f32(3))
    mx = reduce_history(rows, "max")
    assert mx[0] == f32(1e8) and mx[2] == 1.5 and np.isnan(mx[3]) and np.isnan(mx[4])          # NaN if any term is NaN
    assert mx[1] == 0 and not np.signbit(mx[1])                                                # a zero result is +0.0
    assert not np.signbit(reduce_history(np.array([[-0.0], [-0.0]], dtype=f32), "max")[0])
    one = reduce_history(rows[:1], "mean")
    assert np.array_equal(one.view(np.uint32), rows[0].view(np.uint32))                        # len 1: s / 1


def test_history_csr_sorts_and_drops_duplicates():
    pairs = random_histories(12, 60)
    indptr, items = history_csr(pairs, 60)
    assert indptr.dtype == np.int64 and items.dtype == np.int32 and indptr.shape == (13,)
    for u in range(12):
        assert items[indptr[u]: indptr[u + 1]].tolist() == sorted({int(i) for v, i in pairs if v == u})
    # a pair given twice counts once, the order of the pairs does not matter, a ready CSR is taken (and sorted) too
    twice = np.concatenate([pairs[::-1], pairs[:9]])
    again = history_csr(twice, 60)
    assert np.array_equal(again[0], indptr) and np.array_equal(again[1], items)
    unsorted = (np.array([0, 3, 3, 5]), np.array([7, 2, 7, 9, 4], dtype=np.int32))
    got = history_csr(unsorted, 60)
    assert got[0].tolist() == [0, 2, 2, 4] and got[1].tolist() == [2, 7, 4, 9]
    t = U.integer_table(8, 60)
    users = np.arange(12)
    for agg in AGGS:
        a, b = history_scores_host(t, pairs, users, agg, "dot"), history_scores_host(t, twice, users, agg, "dot")
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert np.array_equal(history_scores_host(t, (indptr, items), users, agg, "dot").view(np.uint32), a.view(np.uint32))
    # its own result is handed back as it is (the drivers build the CSR once), unless the table or the ids it is asked for differ
    built = history_csr(pairs, 60)
    assert history_csr(built, 60) is built and history_csr(built, 60, 12) is built
    with pytest.raises(ValueError, match=r"histories: indptr \(13,\) must be \[user_num \+ 1 = 14\]"):
        history_csr(built, 60, 13)
    with pytest.raises(ValueError, match=r"histories: history items in \[0, 58\] outside \[0, 50\)"):
        history_csr(built, 50)
    # the user ids run to the largest user of the pairs, or to what the caller says
    assert history_csr([(4, 1)], 60)[0].tolist() == [0, 0, 0, 0, 0, 1] and len(history_csr([(4, 1)], 60, 9)[0]) == 10


@pytest.mark.parametrize("agg", AGGS)
@pytest.mark.parametrize("metric", ("cosine", "dot"))
def test_the_planted_table_host(agg, metric):
    t, hist, held = planted_world()
    found, scores = recommend_from_history(t, hist, k=4, agg=agg, metric=metric, impl="host")
    assert found.shape == (8, 4) and found.dtype == np.int64 and scores.dtype == np.float32
    full = history_scores_host(t, hist, np.arange(8), agg, metric)
    gap = np.inf
    for c in range(8):
        assert sorted(found[c, :2].tolist()) == [5 * c + 1, 5 * c + 4]          # the two held-out items are the top 2
        assert not set(found[c].tolist()) & {5 * c, 5 * c + 2, 5 * c + 3}       # the history is excluded
        assert (np.diff(scores[c]) <= 0).all() and np.array_equal(scores[c], full[c, found[c]])
        gap = min(gap, float(scores[c, 1] - scores[c, 2]))
    # the smallest gap between the second and the third score: 0.76 under the cosine, 0.68 under the dot product; no rounding closes it
    assert gap >= (0.7 if metric == "cosine" else 0.6), gap
    res, rec = evaluate_history(t, hist, held, ks=(10, 20), agg=agg, metric=metric, impl="host", per_user=True)
    assert list(res) == ["n10", "n20", "r10", "r20", "hr10", "hr20", "mrr", "users", "pairs"]
    assert res["r10"] == 1.0 and res["n10"] == 1.0 and res["hr10"] == 1.0 and res["mrr"] == 1.0 and res["users"] == 8 and res["pairs"] == 16
    assert sorted(rec["ranks"].tolist()) == [1] * 8 + [2] * 8 and np.array_equal(rec["users"], np.arange(8))
    # the pieces by hand, in one batch and in several
    h = heldout_csr(held, 8, 40)
    e = history_csr(hist, 40)
    ranks, flags = heldout_ranks_host(full, np.arange(8), h, e)
    m = catalogue_metrics_host(ranks, h[0], (10, 20))
    assert not flags.any() and np.array_equal(rec["ranks"], ranks) and res["n10"] == m["sums"]["ndcg"][10] / 8
    want = topk_host(full, 4, e[0], e[1], np.arange(8))
    assert np.array_equal(found, want[0]) and np.array_equal(scores, want[1])
    assert evaluate_history(t, hist, held, agg=agg, metric=metric, impl="host", batch_users=3) == res
    cut = recommend_from_history(t, hist, k=4, agg=agg, metric=metric, impl="host", batch_users=3)
    assert np.array_equal(cut[0], found) and np.array_equal(cut[1], scores)
    # a duplicated pair counts once; the order of the pairs does not matter; a ready CSR; chosen users, in their order
    mixed = np.concatenate([hist[::-1], hist[:5]])
    again = recommend_from_history(t, mixed, k=4, agg=agg, metric=metric, impl="host")
    assert np.array_equal(again[0], found) and np.array_equal(again[1].view(np.uint32), scores.view(np.uint32))
    assert evaluate_history(t, mixed, np.concatenate([held, held[:3]]), agg=agg, metric=metric, impl="host") == res
    some = recommend_from_history(t, e, users=[6, 1, 6], k=4, agg=agg, metric=metric, impl="host")
    assert np.array_equal(some[0], found[[6, 1, 6]]) and np.array_equal(some[1], scores[[6, 1, 6]])
    # nothing excluded: the history itself leads (an item is its own nearest); an exclusion list of pairs
    if metric == "cosine" and agg == "max":
        own = recommend_from_history(t, hist, k=3, agg=agg, exclude=None, impl="host")[0]
        assert all(sorted(own[c].tolist()) == [5 * c, 5 * c + 2, 5 * c + 3] for c in range(8))
    gone = recommend_from_history(t, hist, users=[2], k=40, agg=agg, metric=metric, exclude=[(2, 11), (2, 14)], impl="host")[0][0]
    assert not {11, 14} & set(gone.tolist()) and {10, 12, 13} <= set(gone.tolist()) and gone[-2:].tolist() == [-1, -1]


def test_refusals():
    t, hist, held = planted_world()
    for call in (lambda **kw: recommend_from_history(t, hist, **kw), lambda **kw: evaluate_history(t, hist, held, **kw)):
        with pytest.raises(ValueError, match="impl='cpu'"):
            call(impl="cpu")
        with pytest.raises(ValueError, match="metric='l2'"):
            call(metric="l2", impl="host")
        with pytest.raises(ValueError, match="agg='sum'"):
            call(agg="sum", impl="host")
        with pytest.raises(ValueError, match="batch_users = 0"):
            call(batch_users=0, impl="host")
        with pytest.raises(ValueError, match=r"exclude: excluded items in \[-1, -1\] outside"):
            call(exclude=[(0, -1)], impl="host")
        with pytest.raises(ValueError, match=r"exclude: users in \[8, 8\] outside \[0, 8\)"):
            call(exclude=[(8, 1)], impl="host")
        with pytest.raises(ValueError, match="exclude='mine'"):
            call(exclude="mine", impl="host")
    with pytest.raises(ValueError, match="agg='sum'"):
        history_scores_host(t, hist, [0], "sum")
    wide = np.zeros((2, 1025), dtype=np.float32)
    with pytest.raises(ValueError, match=r"recommend_from_history: d = 1025 outside \[1, 1024\]"):
        recommend_from_history(wide, [(0, 1)], impl="host")
    with pytest.raises(ValueError, match=r"evaluate_history: d = 1025 outside \[1, 1024\]"):
        evaluate_history(wide, [(0, 1)], [(0, 0)], impl="host")
    with pytest.raises(ValueError, match="recommend_from_history: the table must be an fp32 array"):
        recommend_from_history(t.astype(np.float64), hist, impl="host")
    for k in (0, 1025, 2.5, True):
        with pytest.raises(ValueError, match="k = "):
            recommend_from_history(t, hist, k=k, impl="host")
    # ids outside the table or the CSR
    with pytest.raises(ValueError, match=r"histories: history items in \[0, 40\] outside \[0, 40\)"):
        recommend_from_history(t, [(0, 40), (1, 0)], impl="host")
    with pytest.raises(ValueError, match=r"histories: users in \[-1, 0\] outside"):
        recommend_from_history(t, [(0, 3), (-1, 0)], impl="host")
    with pytest.raises(ValueError, match=r"histories: history items in \[3, 41\] outside \[0, 40\)"):
        recommend_from_history(t, (np.array([0, 1, 2]), np.array([3, 41], dtype=np.int32)), impl="host")
    with pytest.raises(ValueError, match="histories: indptr must be non-decreasing"):
        recommend_from_history(t, (np.array([0, 2, 1]), np.array([3], dtype=np.int32)), impl="host")
    with pytest.raises(ValueError, match="histories: expected .user, item. integer pairs"):
        recommend_from_history(t, np.zeros((3, 3), dtype=np.int64), impl="host")
    with pytest.raises(ValueError, match="histories: no history at all"):
        recommend_from_history(t, [], impl="host")
    with pytest.raises(ValueError, match=r"recommend_from_history: users in \[8, 8\] outside \[0, 8\)"):
        recommend_from_history(t, hist, users=[8], impl="host")
    with pytest.raises(ValueError, match=r"users .* must be \[U >= 1\]"):
        recommend_from_history(t, hist, users=[], impl="host")
    with pytest.raises(ValueError, match=r"heldout: users in \[8, 8\] outside \[0, 8\)"):
        evaluate_history(t, hist, [(8, 1)], impl="host")
    with pytest.raises(ValueError, match=r"heldout: held-out items in \[40, 40\] outside \[0, 40\)"):
        evaluate_history(t, hist, [(0, 40)], impl="host")
    # a queried user with an empty history
    gap = hist[hist[:, 0] != 3]
    with pytest.raises(ValueError, match="recommend_from_history: 2 of 3 users have an empty history"):
        recommend_from_history(t, gap, users=[3, 0, 3], impl="host")
    assert recommend_from_history(t, gap, k=1, impl="host")[0].shape == (7, 1)      # users=None: those with a history
    with pytest.raises(ValueError, match="evaluate_history: 1 of 8 users have an empty history"):
        evaluate_history(t, gap, held, impl="host")
    with pytest.raises(ValueError, match="history_scores_host: 1 of 1 users have an empty history"):
        history_scores_host(t, gap, [3])
    # the held-out set
    with pytest.raises(ValueError, match="ks="):
        evaluate_history(t, hist, held, ks=(20, 10), impl="host")
    with pytest.raises(ValueError, match="the held-out set is empty"):
        evaluate_history(t, hist, [], impl="host")
    with pytest.raises(ValueError, match="evaluate_history: 2 of 17 held-out pairs are also excluded"):
        evaluate_history(t, hist, np.concatenate([held, [(0, 0)]]), exclude=[(0, 0), (1, 6), (1, 7)], impl="host")
    with pytest.raises(ValueError, match="evaluate_history: 1 of 1 held-out pairs are also excluded"):
        evaluate_history(t, hist, [(0, 2)], impl="host")     # a held-out item of the history meets exclude="history"
    # a NaN: in column x for everybody, in every score of the users who hold x
    bad = np.array(t)
    bad[4, 1] = np.nan
    with pytest.raises(ValueError, match="recommend_from_history: 2 of 3 users have a NaN score among their eligible items"):
        recommend_from_history(bad, hist, users=[0, 1, 2], exclude=[(1, 4)], impl="host")
    recommend_from_history(bad, hist, users=[1, 2], exclude=[(1, 4), (2, 4)], impl="host")      # excluded for all: no error
    with pytest.raises(ValueError, match="evaluate_history: 8 of 8 users have a NaN score among their eligible items"):
        evaluate_history(bad, hist, held, impl="host")
    bad = np.array(t)
    bad[5, 0] = np.nan                                       # an item of user 1's history (excluded with it): every score of user 1
    with pytest.raises(ValueError, match="recommend_from_history: 1 of 2 users have a NaN score among their eligible items"):
        recommend_from_history(bad, hist, users=[1, 2], exclude=[(1, 5), (2, 5)], impl="host")


def test_the_entry_is_declared_bound_and_built():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "pmgt_capi.h")).read()
    assert re.search(r"\bpmgt_history_score\(", hdr) and "pmgt_history_score" in _lib.HIP_SYMBOLS
    assert any(p.endswith(os.path.join("ops", "history_score.hip")) for p in _build.OPS_SOURCES)
    assert "#define PMGT_HISTORY_MEAN 0" in hdr and "#define PMGT_HISTORY_MAX 1" in hdr and _lib.HISTORY_AGGS == ("mean", "max")
    import pmgt_amd
    for name in ("HistoryScorer", "history_scores_host", "recommend_from_history", "evaluate_history"):
        assert name in pmgt_amd.__all__ and hasattr(pmgt_amd, name)
    assert pmgt_amd.HistoryScorer.ids_name == "users"
