"""The numpy side of the truncated, weighted item-kNN: item_knn_scores_host against rows written out by hand and against an independent dense
restatement, the prefix property of the index, weighted_history_csr, decay_weights, recommend_item_knn / evaluate_item_knn(impl="host")
against topk_host / heldout_ranks_host on the dense rows, and every refusal.  No GPU."""
import functools
import os
import re

import numpy as np
import pytest

from pmgt_amd import _build, _lib
from pmgt_amd.catalogue_eval import catalogue_metrics_host, heldout_csr, heldout_ranks_host
from pmgt_amd.history import history_csr
from pmgt_amd.item_knn import (ItemKnnIndex, build_item_knn, decay_weights, evaluate_item_knn, item_knn_scores_host, recommend_item_knn,
                               weighted_history_csr)
from pmgt_amd.recommend import topk_host
from pmgt_amd.similar import item_sim_host
from tests import item_sim_util as U

f32 = np.float32
N_ITEMS, N_USERS = 300, 24
MS = (1, 5, 64, 299, 400)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def world():
    """the table [300, 33], the host index at the largest m (400 > I - 1: padded rows), histories of 1 + (u mod 7) items in no order with one
    weight per pair, and two held-out items a user outside the history; read-only"""
    table = U.normal_table(33, 29)
    index = build_item_knn(table, MS[-1], impl="host", batch_items=77)
    rng = np.random.default_rng(3)
    pairs, held = [], []
    for u in range(N_USERS):
        picks = rng.choice(N_ITEMS, size=3 + u % 7, replace=False)
        pairs += [(u, int(i)) for i in picks[2:]]
        held += [(u, int(i)) for i in picks[:2]]
    pairs = np.array(pairs, dtype=np.int64)[rng.permutation(len(pairs))]
    weights = rng.uniform(0.25, 5.0, size=len(pairs)).astype(np.float32)
    for a in (table, pairs, weights):
        a.setflags(write=False)
    return table, index, pairs, weights, np.array(held, dtype=np.int64)


def dense_restatement(index, m, pairs, weights, users):
    """AN INDEPENDENT RESTATEMENT: the index scattered into an [I, I] matrix (0 where j is not listed, with a mask of what is listed), then per
    candidate the history rows gathered and added in the order of the sorted history, every operation in np.float32"""
    n = index.n_items
    nbr, sim = index.nbr[:, :m], index.sim[:, :m]
    dense, listed = np.zeros((n, n), dtype=f32), np.zeros((n, n), dtype=bool)
    for i in range(n):
        for c in range(nbr.shape[1]):
            if nbr[i, c] >= 0:
                dense[i, nbr[i, c]], listed[i, nbr[i, c]] = sim[i, c], True
    out = np.zeros((len(users), n), dtype=f32)
    for r, u in enumerate(users):
        mine = sorted((int(i), k) for k, (v, i) in enumerate(pairs) if v == u)
        for j in range(n):
            acc = f32(0)
            for i, k in mine:
                if listed[i, j]:
                    term = dense[i, j] if weights is None else f32(f32(weights[k]) * dense[i, j])
                    acc = f32(acc + term)
            out[r, j] = acc
    return out


def test_the_rows_written_out_by_hand():
    """5 items, m = 2, two users: item 4 is listed by nobody, row 3 has one neighbour and a padded slot"""
    nbr = np.array([[1, 2], [0, 2], [1, 0], [2, -1], [0, 1]], dtype=np.int32)
    sim = np.array([[0.5, 0.25], [0.5, 0.125], [0.75, 0.25], [2.0, -np.inf], [1.0, -1.0]], dtype=f32)
    index = ItemKnnIndex(nbr, sim, 5)
    assert index.m == 2 and index.stride == 2 and index.n_items == 5 and not index.on_device
    hist = [(0, 3), (0, 0), (1, 4), (1, 1), (1, 2)]          # user 0: items 0, 3; user 1: items 1, 2, 4
    got = item_knn_scores_host(index, hist, [0, 1])
    # user 0: item 0 lists 1 (.5) and 2 (.25); item 3 lists 2 (2.)      user 1: 1 lists 0 (.5), 2 (.125); 2 lists 1 (.75), 0 (.25); 4 lists 0 (1), 1 (-1)
    want = np.array([[0.0, 0.5, 2.25, 0.0, 0.0], [1.75, -0.25, 0.125, 0.0, 0.0]], dtype=f32)
    assert got.dtype == np.float32 and np.array_equal(bits(got), bits(want))      # (+0.0 where nobody lists the item)
    w = [2.0, 3.0, 0.5, 1.0, -1.0]                           # aligned with the pairs as given
    got = item_knn_scores_host(index, hist, [1, 0], weights=w)
    want = np.array([[0.5 - 0.25 + 0.5, -0.75 - 0.5, 0.125, 0.0, 0.0], [0.0, 1.5, 0.75 + 4.0, 0.0, 0.0]], dtype=f32)
    assert np.array_equal(bits(got), bits(want))
    # m = 1: the first column alone
    got = item_knn_scores_host(index, hist, [0, 1], m=1)
    assert np.array_equal(bits(got), bits(np.array([[0, 0.5, 2.0, 0, 0], [1.5, 0.75, 0, 0, 0]], dtype=f32)))
    # a zero result is +0.0: 0.75 - 0.75
    zero = ItemKnnIndex(np.array([[1], [0], [1]], dtype=np.int32), np.array([[1.0], [1.0], [-1.0]], dtype=f32), 3)
    z = item_knn_scores_host(zero, [(0, 0), (0, 2)], [0])
    assert z[0, 1] == 0 and not np.signbit(z[0]).any()
    z = item_knn_scores_host(zero, [(0, 0), (0, 2)], [0], weights=[-0.0, 0.0])      # -0.0 terms on +0.0
    assert (z == 0).all() and not np.signbit(z).any()


@pytest.mark.parametrize("weighted", (False, True))
def test_the_yardstick_is_the_dense_restatement(weighted):
    table, index, pairs, weights, _ = world()
    users = np.array([3, 0, 23, 3, 6, 13], dtype=np.int64)
    w = weights if weighted else None
    for m in MS:
        got = item_knn_scores_host(index, pairs, users, w, m)
        want = dense_restatement(index, m, pairs, w, users)
        assert got.shape == (6, N_ITEMS) and np.array_equal(bits(got), bits(want)), m
    full = item_knn_scores_host(index, pairs, users, w)      # m None: all the index has
    assert np.array_equal(bits(full), bits(item_knn_scores_host(index, pairs, users, w, MS[-1])))
    # m = 299 is the whole catalogue but the item itself; 400 adds padding only
    assert np.array_equal(bits(full), bits(item_knn_scores_host(index, pairs, users, w, 299)))
    # a ready CSR (with the weights carried through the sort) gives the same rows
    csr, cw = (history_csr(pairs, N_ITEMS), None) if w is None else weighted_history_csr(pairs, w, N_ITEMS)
    assert np.array_equal(bits(item_knn_scores_host(index, csr, users, cw, 5)), bits(item_knn_scores_host(index, pairs, users, w, 5)))


def test_the_index_as_built_on_the_host():
    table, index, *_ = world()
    assert index.nbr.dtype == np.int32 and index.sim.dtype == np.float32 and index.nbr.shape == (N_ITEMS, 400) and index.m == 400
    nbr, sim = index.nbr, index.sim
    assert (nbr[:, :299] >= 0).all() and (nbr[:, 299:] == -1).all() and np.isneginf(sim[:, 299:]).all()      # I - 1 < m: the padding
    assert not (nbr[:, :299] == np.arange(N_ITEMS)[:, None]).any()      # item i itself is excluded
    assert all(len(set(row[:299].tolist())) == 299 for row in nbr)
    assert (np.diff(sim[:, :299], axis=1) <= 0).all()        # best first
    ItemKnnIndex(nbr, sim, N_ITEMS)                          # what the builder makes passes the checks of arrays from elsewhere
    # THE PREFIX PROPERTY: truncated(m2) is the index built at m2 (the same batch: the host sums are BLAS's and move with it)
    for m2 in (1, 5, 64):
        small = build_item_knn(table, m2, impl="host", batch_items=77)
        cut = index.truncated(m2)
        assert cut.m == m2 and cut.stride == 400 and cut.nbr.shape == (N_ITEMS, m2)
        assert np.array_equal(small.nbr, cut.nbr) and np.array_equal(bits(small.sim), bits(cut.sim))
        _, _, pairs, weights, _ = world()
        a = item_knn_scores_host(cut, pairs, np.arange(N_USERS), weights)
        b = item_knn_scores_host(small, pairs, np.arange(N_USERS), weights)
        assert np.array_equal(bits(a), bits(b))
    assert index.truncated(400).truncated(7).m == 7 and index.host() is index
    dot = build_item_knn(table[:40], 3, metric="dot", impl="host")
    row = item_sim_host(table[:40], None, "dot")[0]          # (one batch, as the builder's: the sums are BLAS's)
    assert dot.nbr.shape == (40, 3) and np.array_equal(dot.sim[0], np.sort(row[1:])[::-1][:3]) and np.array_equal(row[dot.nbr[0]], dot.sim[0])


def test_weighted_history_csr():
    pairs = np.array([(2, 5), (0, 9), (2, 1), (0, 3), (2, 3)], dtype=np.int64)
    w = np.array([1.0, 2.0, 3.0, 4.0, 5.0])
    csr, cw = weighted_history_csr(pairs, w, 10)
    assert csr[0].tolist() == [0, 2, 2, 5] and csr[1].tolist() == [3, 9, 1, 3, 5] and csr[1].dtype == np.int32
    assert cw.dtype == np.float32 and cw.tolist() == [4.0, 2.0, 3.0, 5.0, 1.0]      # carried through the sort
    plain = history_csr(pairs, 10)
    assert np.array_equal(plain[0], csr[0]) and np.array_equal(plain[1], csr[1])
    again, aw = weighted_history_csr(csr, cw, 10)             # its own result, and any ready CSR pair with aligned weights
    assert np.array_equal(again[1], csr[1]) and np.array_equal(aw, cw)
    unsorted = (np.array([0, 2, 2, 3]), np.array([7, 2, 4], dtype=np.int32))
    got, gw = weighted_history_csr(unsorted, [1.0, 2.0, 3.0], 10, 3)
    assert got[0].tolist() == [0, 2, 2, 3] and got[1].tolist() == [2, 7, 4] and gw.tolist() == [2.0, 1.0, 3.0]
    with pytest.raises(ValueError, match="1 .user, item. pairs are given more than once"):
        weighted_history_csr(np.concatenate([pairs, pairs[:1]]), np.ones(6), 10)
    with pytest.raises(ValueError, match="1 of 5 weights are not finite"):
        weighted_history_csr(pairs, [1, 2, np.nan, 4, 5], 10)
    with pytest.raises(ValueError, match="1 of 5 weights are not finite"):
        weighted_history_csr(pairs, [1, 2, 1e39, 4, 5], 10)  # finite in fp64, not in fp32
    with pytest.raises(ValueError, match=r"weights \(4,\) must be \[5\]"):
        weighted_history_csr(pairs, np.ones(4), 10)
    with pytest.raises(ValueError, match=r"histories: history items in \[1, 9\] outside \[0, 9\)"):
        weighted_history_csr(pairs, w, 9)
    with pytest.raises(ValueError, match="histories: no history at all"):
        weighted_history_csr([], [], 10)


def test_decay_weights_against_the_formula_written_out():
    users = np.array([7, 2, 7, 9, 2, 7], dtype=np.int64)
    times = np.array([100.0, 50.0, 130.0, 5.0, 20.0, 70.0])
    got = decay_weights(users, times, 30.0)
    want = [0.5 ** ((130.0 - 100.0) / 30.0), 1.0, 1.0, 1.0, 0.5 ** ((50.0 - 20.0) / 30.0), 0.5 ** ((130.0 - 70.0) / 30.0)]
    assert got.dtype == np.float32 and np.array_equal(got, np.array(want, dtype=np.float64).astype(np.float32))
    assert got.tolist() == [0.5, 1.0, 1.0, 1.0, 0.5, 0.25]
    odd = decay_weights([0, 0], [0, 7], 3.0)
    assert odd[0] == np.float32(0.5 ** (7.0 / 3.0)) and odd[1] == 1.0      # fp64, rounded once
    for bad in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(ValueError, match="half_life"):
            decay_weights(users, times, bad)
    with pytest.raises(ValueError, match="decay_weights: users"):
        decay_weights(users[:3], times, 1.0)


@pytest.mark.parametrize("weighted", (False, True))
def test_recommend_and_evaluate_on_the_host_are_the_pieces_on_the_dense_rows(weighted):
    table, index, pairs, weights, held = world()
    w = weights if weighted else None
    users = np.arange(N_USERS, dtype=np.int64)
    e = history_csr(pairs, N_ITEMS)
    h = heldout_csr(held, N_USERS, N_ITEMS)
    for m in (5, 64):
        rows = dense_restatement(index, m, pairs, w, users)
        found, scores = recommend_item_knn(index, pairs, k=20, m=m, weights=w, impl="host")
        want = topk_host(rows, 20, e[0], e[1], users)
        assert found.dtype == np.int64 and np.array_equal(found, want[0]) and np.array_equal(bits(scores), bits(want[1]))
        cut = recommend_item_knn(index, pairs, users=[6, 1, 6], k=20, m=m, weights=w, impl="host", batch_users=2, exclude=None)
        want = topk_host(rows[[6, 1, 6]], 20)
        assert np.array_equal(cut[0], want[0]) and np.array_equal(bits(cut[1]), bits(want[1]))
        res, rec = evaluate_item_knn(index, pairs, held, ks=(10, 20), m=m, weights=w, impl="host", per_user=True, batch_users=7)
        ranks, flags = heldout_ranks_host(rows, users, h, e)
        met = catalogue_metrics_host(ranks, h[0], (10, 20))
        assert not flags.any() and np.array_equal(rec["ranks"], ranks) and res["n10"] == met["sums"]["ndcg"][10] / N_USERS
        assert list(res) == ["n10", "n20", "r10", "r20", "hr10", "hr20", "mrr", "users", "pairs"] and res["pairs"] == 2 * N_USERS
        assert evaluate_item_knn(index, pairs, held, m=m, weights=w, impl="host") == res
    # a user with fewer than k eligible items: m = 1 lists at most one item per history item, the rest tie at +0.0 and still rank; with the
    # whole catalogue excluded but two items the padding shows
    most = [(0, j) for j in range(N_ITEMS) if j not in (7, 250)]
    short = recommend_item_knn(index, pairs, users=[0], k=4, m=1, weights=w, exclude=most, impl="host")
    assert short[0][0, 2:].tolist() == [-1, -1] and sorted(short[0][0, :2].tolist()) == [7, 250] and np.isneginf(short[1][0, 2:]).all()


def test_the_tuple_m_form_equals_the_separate_calls_and_a_table_builds_its_index():
    table, index, pairs, weights, held = world()
    sweep = evaluate_item_knn(index, pairs, held, m=(1, 5, 64), weights=weights, impl="host", per_user=True)
    assert list(sweep) == [1, 5, 64]
    for m in (1, 5, 64):
        res, rec = evaluate_item_knn(index, pairs, held, m=m, weights=weights, impl="host", per_user=True)
        assert sweep[m][0] == res and np.array_equal(sweep[m][1]["ranks"], rec["ranks"])
        assert evaluate_item_knn(index.truncated(m), pairs, held, weights=weights, impl="host") == res      # m None: all the index has
    assert len({tuple(sweep[m][1]["ranks"].tolist()) for m in sweep}) == 3      # m is a hyper-parameter: the ranks move with it
    assert evaluate_item_knn(index, pairs, held, m=(5,), impl="host") == {5: evaluate_item_knn(index, pairs, held, m=5, impl="host")}
    # a table in the first place builds the index (cosine, m or 64) on the side impl names
    t = U.planted_table()
    hist = np.array([(c, 5 * c + a) for c in range(8) for a in (0, 2, 3)], dtype=np.int64)
    held = np.array([(c, 5 * c + a) for c in range(8) for a in (1, 4)], dtype=np.int64)
    found, scores = recommend_item_knn(t, hist, k=4, m=4, impl="host")
    assert all(sorted(found[c, :2].tolist()) == [5 * c + 1, 5 * c + 4] for c in range(8))      # the cluster's two other items lead
    by_index = recommend_item_knn(build_item_knn(t, 4, impl="host"), hist, k=4, impl="host")
    assert np.array_equal(found, by_index[0]) and np.array_equal(bits(scores), bits(by_index[1]))
    res = evaluate_item_knn(t, hist, held, m=(2, 4), impl="host")
    assert res[4]["r10"] == 1.0 and res[4]["mrr"] == 1.0 and res[4] == evaluate_item_knn(t, hist, held, m=4, impl="host")
    assert evaluate_item_knn(t, hist, held, impl="host") == evaluate_item_knn(build_item_knn(t, 64, impl="host"), hist, held, impl="host")


def test_refusals():
    table, index, pairs, weights, held = world()
    calls = (lambda **kw: recommend_item_knn(index, pairs, **kw), lambda **kw: evaluate_item_knn(index, pairs, held, **kw))
    for call, who in zip(calls, ("recommend_item_knn", "evaluate_item_knn")):
        with pytest.raises(ValueError, match="impl='cpu'"):
            call(impl="cpu")
        for m in (0, 1025, 2.5, True):
            with pytest.raises(ValueError, match="m = "):
                call(m=m, impl="host")
        with pytest.raises(ValueError, match=f"{who}: m = 401 is larger than the 400 neighbours the index has"):
            call(m=401, impl="host")
        with pytest.raises(ValueError, match=r"weights \(3,\) must be \[%d\]" % len(pairs)):
            call(weights=np.ones(3), impl="host")
        with pytest.raises(ValueError, match="weights are not finite"):
            call(weights=np.where(np.arange(len(pairs)) == 4, np.inf, 1.0), impl="host")
        with pytest.raises(ValueError, match="batch_users = 0"):
            call(batch_users=0, impl="host")
        with pytest.raises(ValueError, match=r"exclude: excluded items in \[300, 300\] outside"):
            call(exclude=[(0, 300)], impl="host")
        with pytest.raises(ValueError, match="exclude='mine'"):
            call(exclude="mine", impl="host")
    twice = np.concatenate([pairs, pairs[:2]])
    with pytest.raises(ValueError, match="2 .user, item. pairs are given more than once"):
        recommend_item_knn(index, twice, weights=np.ones(len(twice)), impl="host")
    assert np.array_equal(recommend_item_knn(index, twice, impl="host")[0], recommend_item_knn(index, pairs, impl="host")[0])      # without weights: once
    for k in (0, 1025, 2.5, True):
        with pytest.raises(ValueError, match="k = "):
            recommend_item_knn(index, pairs, k=k, impl="host")
    with pytest.raises(ValueError, match="recommend_item_knn: m must be one size"):
        recommend_item_knn(index, pairs, m=(1, 5), impl="host")
    with pytest.raises(ValueError, match="must be ascending sizes"):
        evaluate_item_knn(index, pairs, held, m=(5, 5), impl="host")
    with pytest.raises(ValueError, match="must be ascending sizes"):
        evaluate_item_knn(index, pairs, held, m=(), impl="host")
    # ids outside the table or the CSR, a queried user with an empty history
    with pytest.raises(ValueError, match=r"histories: history items in \[0, 300\] outside \[0, 300\)"):
        recommend_item_knn(index, [(0, 300), (1, 0)], impl="host")
    with pytest.raises(ValueError, match=r"histories: users in \[-1, 0\] outside"):
        recommend_item_knn(index, [(0, 3), (-1, 0)], impl="host")
    with pytest.raises(ValueError, match=r"recommend_item_knn: users in \[24, 24\] outside \[0, 24\)"):
        recommend_item_knn(index, pairs, users=[24], impl="host")
    gap = pairs[pairs[:, 0] != 3]
    with pytest.raises(ValueError, match="recommend_item_knn: 2 of 3 users have an empty history"):
        recommend_item_knn(index, gap, users=[3, 0, 3], impl="host")
    assert recommend_item_knn(index, gap, k=1, impl="host")[0].shape == (N_USERS - 1, 1)      # users=None: those with a history
    with pytest.raises(ValueError, match="evaluate_item_knn: 1 of 24 users have an empty history"):
        evaluate_item_knn(index, gap, held, impl="host")
    with pytest.raises(ValueError, match="item_knn_scores_host: 1 of 1 users have an empty history"):
        item_knn_scores_host(index, gap, [3])
    with pytest.raises(ValueError, match="item_knn_scores_host: m = 401 is larger"):
        item_knn_scores_host(index, pairs, [0], m=401)
    with pytest.raises(ValueError, match="expected an ItemKnnIndex"):
        item_knn_scores_host((index.nbr, index.sim), pairs, [0])
    # the held-out set
    with pytest.raises(ValueError, match="the held-out set is empty"):
        evaluate_item_knn(index, pairs, [], impl="host")
    with pytest.raises(ValueError, match="evaluate_item_knn: 1 of %d held-out pairs are also excluded" % (len(held) + 1)):
        evaluate_item_knn(index, pairs, np.concatenate([held, pairs[:1]]), impl="host")      # an item of the history meets exclude="history"
    with pytest.raises(ValueError, match=r"heldout: users in \[24, 24\] outside \[0, 24\)"):
        evaluate_item_knn(index, pairs, [(24, 1)], impl="host")
    with pytest.raises(ValueError, match="ks="):
        evaluate_item_knn(index, pairs, held, ks=(20, 10), impl="host")
    # the builder
    with pytest.raises(ValueError, match="m = 1025"):
        build_item_knn(table, 1025, impl="host")
    with pytest.raises(ValueError, match="metric='l2'"):
        build_item_knn(table, 5, metric="l2", impl="host")
    with pytest.raises(ValueError, match="impl='gpu'"):
        build_item_knn(table, 5, impl="gpu")
    with pytest.raises(ValueError, match=r"build_item_knn: d = 1025 outside \[1, 1024\]"):
        build_item_knn(np.zeros((2, 1025), dtype=np.float32), 1, impl="host")
    bad = np.array(table[:50])
    bad[4, 1] = np.nan
    with pytest.raises(ValueError, match="build_item_knn: 50 of 50 items have a NaN score among their eligible items"):
        build_item_knn(bad, 5, impl="host")                  # column 4 reaches every row: an index never holds a NaN
    with pytest.raises(ValueError, match=r"recommend_item_knn: d = 1025 outside \[1, 1024\]"):
        recommend_item_knn(np.zeros((2, 1025), dtype=np.float32), [(0, 1)], impl="host")


def test_an_index_from_elsewhere_is_checked():
    nbr = np.array([[1, 2], [0, 2], [1, -1]], dtype=np.int32)
    sim = np.array([[0.5, 0.25], [0.5, 0.125], [0.75, -np.inf]], dtype=f32)
    ItemKnnIndex(nbr, sim, 3)
    ItemKnnIndex(nbr, sim.clip(-9, 9), 3)                    # (what a padded slot holds is not read)

    def broken(at, value, values=sim):
        x = np.array(nbr)
        x[at] = value
        return x, values
    with pytest.raises(ValueError, match="1 of 3 rows repeat a neighbour id"):
        ItemKnnIndex(*broken((0, 1), 1), 3)
    with pytest.raises(ValueError, match=r"neighbour ids in \[-1, 3\] outside \[-1, 3\)"):
        ItemKnnIndex(*broken((0, 1), 3), 3)
    with pytest.raises(ValueError, match=r"neighbour ids in \[-2, 2\] outside"):
        ItemKnnIndex(*broken((0, 1), -2), 3)
    with pytest.raises(ValueError, match="a -1 slot must be followed only by -1 slots"):
        ItemKnnIndex(*broken((0, 0), -1), 3)
    with pytest.raises(ValueError, match="1 similarities in live slots are not finite"):
        ItemKnnIndex(nbr, np.where(np.arange(6).reshape(3, 2) == 2, np.nan, sim).astype(f32), 3)
    with pytest.raises(ValueError, match="must be int32 and fp32"):
        ItemKnnIndex(nbr, sim[:, :1], 3)
    with pytest.raises(ValueError, match="must be int32 and fp32"):
        ItemKnnIndex(nbr.astype(np.int64), sim, 3)
    with pytest.raises(ValueError, match="must be int32 and fp32"):
        ItemKnnIndex(nbr, sim, 4)
    with pytest.raises(ValueError, match="n_items = 0"):
        ItemKnnIndex(nbr, sim, 0)
    with pytest.raises(ValueError, match="m = 3 is larger than the 2 neighbours"):
        ItemKnnIndex(nbr, sim, 3).truncated(3)
    with pytest.raises(ValueError, match="m = 0"):
        ItemKnnIndex(nbr, sim, 3).truncated(0)


def test_the_entry_is_declared_bound_and_built():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "pmgt_capi.h")).read()
    assert re.search(r"\bpmgt_knn_score\(", hdr) and re.search(r"\bpmgt_knn_score_tile\(", hdr)
    assert "pmgt_knn_score" in _lib.HIP_SYMBOLS and "pmgt_knn_score_tile" in _lib.HIP_SYMBOLS
    assert any(p.endswith(os.path.join("ops", "knn_score.hip")) for p in _build.OPS_SOURCES)
    import pmgt_amd
    for name in ("ItemKnnIndex", "ItemKnnScorer", "build_item_knn", "weighted_history_csr", "decay_weights", "item_knn_scores_host",
                 "recommend_item_knn", "evaluate_item_knn"):
        assert name in pmgt_amd.__all__ and hasattr(pmgt_amd, name)
    assert pmgt_amd.ItemKnnScorer.entry == "knn_score" and pmgt_amd.ItemKnnScorer.ids_name == "users"
    assert pmgt_amd.ItemKnnScorer.max_ids == _lib.NCF_MAX_USERS
