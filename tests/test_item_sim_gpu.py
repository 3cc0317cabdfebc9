"""pmgt_item_sim_norms / pmgt_item_sim_score against item_sim_host at the tile's edges: bit for bit where every sum is exact, within the
project's measure where it is rounded; the three properties the score's definition buys (symmetric, independent of the batch, a NaN stays
local); the selection and rank kernels on the kernel's own rows; similar_items / evaluate_neighbours on both impls; the refusals."""
import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd import similar as S
from pmgt_amd.catalogue_eval import CatalogueMetrics, HeldoutRanks, catalogue_metrics_host, heldout_ranks_host
from pmgt_amd.graph import synthetic_graph
from pmgt_amd.recommend import TopkRows, topk_host
from pmgt_amd.similar import (ItemSimScorer, edges_csr, evaluate_neighbours, holdout_edges, item_exclusion_csr, item_sim_host, similar_items)
from tests import item_sim_util as U

pytestmark = pytest.mark.gpu

SENTINEL = 7777.0


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()              # (a copy: the shared arrays are read-only, a reversed view has negative strides)


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def device_scores(table, q, metric, slack=0):
    """the kernel's rows [len(q), I] of the queries q; with `slack`, into a wider buffer whose columns past I must stay as they were"""
    scorer = ItemSimScorer(dev(table), metric)
    n, n_items = len(q), len(table)
    out = torch.full((n + 1, n_items + slack), SENTINEL, dtype=torch.float32, device="cuda")
    got = scorer.score(dev(np.asarray(q, dtype=np.int64)), out=out)
    assert got is out
    x = out.cpu().numpy()
    assert (x[n] == SENTINEL).all() and (x[:, n_items:] == SENTINEL).all()      # the row past n and the columns past I are untouched
    return x[:n, :n_items]


@pytest.mark.parametrize("d", U.EXACT_DS)
def test_exact_case_bit_for_bit(d):
    full = U.integer_table(d)
    for n_items in U.ITEMS:
        table, q = full[:n_items], U.queries_of(n_items)
        want = item_sim_host(table, q, "dot")
        for n in U.NS:
            got = device_scores(table, q[:n], "dot", slack=3)
            assert np.array_equal(bits(got), bits(want[:n])), (n_items, n)


@pytest.mark.parametrize("d", U.EXACT_DS)
def test_exact_case_same_lists_ranks_and_metrics_on_both_impls(d):
    """the integer table is full of ties: the order among them is the lower item index first, on the device as on the host"""
    table = U.integer_table(d)
    n_items = len(table)
    q = U.queries_of(n_items)
    train = synthetic_graph(n_items, 2 * n_items, seed=1)
    for kw in (dict(), dict(exclude=train, batch_items=67), dict(exclude_self=False, batch_items=1000)):
        a = similar_items(table, q, k=20, metric="dot", impl="device", **kw)
        b = similar_items(table, q, k=20, metric="dot", impl="host", **kw)
        assert a[0].dtype == np.int64 and np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1]))
    split, held = holdout_edges(synthetic_graph(n_items, 3 * n_items, seed=2), 0.2, seed=0)
    for kw in (dict(exclude=split), dict(exclude=split, batch_items=33), dict()):
        (ra, pa), (rb, pb) = (evaluate_neighbours(table, held, ks=(1, 10, 20), metric="dot", impl=impl, per_item=True, **kw)
                              for impl in ("device", "host"))
        assert ra == rb and set(pa) == set(pb)
        for key in ("items", "n_pos", "ranks", "indptr", "heldout", "rr"):
            assert np.array_equal(pa[key], pb[key]), key
        for key in ("ndcg", "recall", "hit"):
            for k in (1, 10, 20):
                assert np.array_equal(pa[key][k], pb[key][k]), (key, k)


@pytest.mark.parametrize("d", U.DS)
def test_rounded_case_within_the_measure(d):
    w = U.world(d)
    worst = {}
    for metric in S.METRICS:
        o64, r32 = w[metric]
        for n_items in U.ITEMS:
            table, q = w["table"][:n_items], U.queries_of(n_items)
            for n in U.NS:
                got = device_scores(table, q[:n], metric)
                worst[(metric, n_items, n)] = U.case_ratio(got, o64, r32, q[:n], n_items)
    top = max(worst, key=worst.get)
    print(f"d = {d}: the largest ratio {worst[top]:.3f} at (metric, I, n) = {top}")
    assert worst[top] <= U.C_BOUND, (top, worst[top])


def test_norms_are_the_clamped_inverse_norms():
    for d in U.DS:
        t = np.array(U.world(d)["table"])
        t[3] = 0                                             # the clamp: 1 / eps
        t[5] *= np.float32(1e-20)                            # below eps
        s = ItemSimScorer(dev(t), "cosine")
        got = s.inv_norm.cpu().numpy().astype(np.float64)
        want = 1 / np.maximum(np.sqrt((t.astype(np.float64) ** 2).sum(axis=1)), np.float64(np.float32(1e-12)))
        # a sequential sum of d squares (the dot product's chain), then a square root and a division: at most d roundings in the sum (the
        # terms are positive: each is at most half an ulp of a partial sum below the total), halved by the root, and one each for the
        # root and the quotient
        assert np.abs(got / want - 1).max() <= (d / 2 + 2) * 2.0 ** -24, d
        assert got[3] == np.float32(1) / np.float32(1e-12) and got[5] == got[3]
    assert ItemSimScorer(dev(t), "dot").inv_norm is None
    # the sum of squares is the dot product's own chain: sqrt(dot(j, j)) has the bits of 1 / inv[j] before the division
    for d in (33, 1024):
        t = U.world(d)["table"]
        self_dot = np.diagonal(device_scores(t, np.arange(len(t)), "dot"))
        inv = ItemSimScorer(dev(t), "cosine").inv_norm.cpu().numpy()
        assert np.array_equal(bits(inv), bits(np.float32(1) / np.sqrt(self_dot))), d
        self_cos = np.diagonal(device_scores(t, np.arange(len(t)), "cosine")).astype(np.float64)
        assert np.abs(self_cos - 1).max() <= 6 * 2.0 ** -24, d      # the roundings of sqrt and 1 / x enter twice, those of the two products once


def test_symmetric_batch_independent_and_repeatable():
    t = U.world(100)["table"]
    n_items = len(t)
    for metric in S.METRICS:
        full = device_scores(t, np.arange(n_items), metric)
        assert np.array_equal(bits(full), bits(full.T)), metric                  # s(i, j) and s(j, i): the same bits
        q = U.queries_of(n_items)
        rows = device_scores(t, q, metric)                                       # unordered, one id twice, the 128 x 128 tile
        assert np.array_equal(bits(rows), bits(full[q])) and np.array_equal(bits(rows), bits(device_scores(t, q, metric)))
        for n in (1, 5, 32, 33, 67):                                             # the 32 x 256 tile up to 32, the other above
            assert np.array_equal(bits(device_scores(t, q[:n][::-1], metric)), bits(full[q[:n][::-1]])), (metric, n)
        # the catalogue cut: a shorter table gives the same bits for the pairs it holds
        for cut in (129, 33):
            part = device_scores(t[:cut], np.arange(cut), metric)
            assert np.array_equal(bits(part), bits(full[:cut, :cut])), (metric, cut)


def test_nan_stays_in_its_row_and_column_and_a_zero_row_scores_zero():
    t = np.array(U.world(33)["table"])
    t[70, 32] = np.nan
    t[11] = 0
    clean = np.array(U.world(33)["table"])
    n_items = len(t)
    for metric in S.METRICS:
        x = device_scores(t, np.arange(n_items), metric)
        want = np.zeros((n_items, n_items), bool)
        want[70] = want[:, 70] = True
        assert np.array_equal(np.isnan(x), want), metric
        ok = ~want
        assert (x[11][ok[11]] == 0).all() and (x[:, 11][ok[:, 11]] == 0).all()
        # every other score has the bits of the table without the NaN and the zero row
        ref = device_scores(clean, np.arange(n_items), metric)
        ok[11] = ok[:, 11] = False
        assert np.array_equal(bits(x)[ok], bits(ref)[ok]), metric


def test_a_query_outside_the_table_is_never_read_its_row_is_nan():
    t = U.world(8)["table"][:40]
    s = ItemSimScorer(dev(t), "cosine")
    q = np.array([3, 40, -1, 2 ** 40, 7], dtype=np.int64)
    x = s.score(dev(q)).cpu().numpy()
    assert np.isnan(x[1:4]).all() and not np.isnan(x[[0, 4]]).any()
    assert np.array_equal(bits(x[[0, 4]]), bits(device_scores(t, [3, 7], "cosine")))


def test_selection_and_ranks_on_the_kernels_own_rows():
    t = U.world(100)["table"]
    n_items = len(t)
    q = U.queries_of(n_items)
    train, held = holdout_edges(synthetic_graph(n_items, 3 * n_items, seed=3), 0.2, seed=1)
    e = item_exclusion_csr(train, n_items, True)
    h = edges_csr(held, n_items, True, "heldout")
    scorer = ItemSimScorer(dev(t), "cosine")
    q_d = dev(q)
    rows = scorer.score(q_d)
    x = rows.cpu().numpy()
    # top-k
    got = TopkRows("cuda", len(q), n_items, 20, *e, n_items).select(rows, q_d)
    want = topk_host(x, 20, *e, q)
    assert np.array_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(bits(got[1].cpu().numpy()), bits(want[1]))
    assert np.array_equal(got[2].cpu().numpy().view(np.uint32), want[2])
    # ranks and metrics: the evaluated queries are the items with a held-out neighbour
    ev = np.nonzero(np.diff(h[0]) > 0)[0].astype(np.int64)
    ev_d = dev(ev)
    rows = scorer.score(ev_d)
    ranker = HeldoutRanks("cuda", n_items, *h, n_items, *e)
    flags = torch.zeros(len(ev), dtype=torch.int32, device="cuda")
    ranker.rank(rows, ev_d, flags)
    reducer = CatalogueMetrics("cuda", len(ev), (10, 20))
    reducer.reduce(ranker, ev_d, flags)
    ranks, host_flags = heldout_ranks_host(rows.cpu().numpy(), ev, h, e)
    m = catalogue_metrics_host(ranks, h[0], (10, 20))
    assert np.array_equal(ranker.ranks.cpu().numpy(), ranks) and not host_flags.any() and not flags.cpu().numpy().any()
    rec, st = reducer.per_user(), reducer.statistic()
    for k in (10, 20):
        for key in ("ndcg", "recall", "hit"):
            assert np.array_equal(rec[key][k], m[key][k]) and st[key][k] == m["sums"][key][k], (key, k)
    assert np.array_equal(rec["rr"], m["rr"]) and st["rr"] == m["sums"]["rr"] and st["n_users"] == len(ev)


def test_end_to_end_on_the_planted_table():
    t = U.planted_table()
    train, held = holdout_edges(synthetic_graph(U.PLANTED_ITEMS, 3 * U.PLANTED_ITEMS, seed=5), 0.25, seed=0)
    assert len(held) == 30
    for table in (np.array(t), dev(t)):                      # a numpy array is uploaded once; a device tensor is read in place
        for kw in (dict(), dict(batch_items=7)):
            (ra, pa), (rb, pb) = (evaluate_neighbours(table, held, exclude=train, ks=(5, 10), impl=impl, per_item=True, **kw)
                                  for impl in ("device", "host"))
            assert list(ra) == ["n5", "n10", "r5", "r10", "hr5", "hr10", "mrr", "items", "pairs"]
            assert ra["items"] == rb["items"] and ra["pairs"] == rb["pairs"] == 60
            for key in ("items", "n_pos", "ranks", "indptr", "heldout", "rr"):
                assert np.array_equal(pa[key], pb[key]), key
            for key in ("ndcg", "recall", "hit"):
                for k in (5, 10):
                    assert np.array_equal(pa[key][k], pb[key][k]), (key, k)
            assert ra == rb
    # the planted clusters: held-out edges inside them land within the cluster
    res, rec = evaluate_neighbours(dev(t), U.planted_edges(), ks=(4, 10), per_item=True)
    assert res["r10"] == 1.0 and rec["ranks"].max() <= 4
    found, scores = similar_items(dev(t), k=6)
    host_found, host_scores = similar_items(t, k=6, impl="host")
    assert np.array_equal(found, host_found) and np.abs(scores - host_scores).max() <= 2.0 ** -22


def test_refusals_come_before_any_launch(monkeypatch):
    class NoLaunch:
        def __init__(self, *a, **kw):
            raise AssertionError("a scorer was built")
    monkeypatch.setattr(S, "ItemSimScorer", NoLaunch)
    monkeypatch.setattr(S, "device_table", NoLaunch)
    t, edges = dev(U.planted_table()), U.planted_edges()
    for call in (lambda **kw: similar_items(t, [0], **kw), lambda **kw: evaluate_neighbours(t, edges, **kw)):
        with pytest.raises(ValueError, match="impl='gpu'"):
            call(impl="gpu")
        with pytest.raises(ValueError, match="metric='l2'"):
            call(metric="l2")
        with pytest.raises(ValueError, match="batch_items = -1"):
            call(batch_items=-1)
        with pytest.raises(ValueError, match=r"exclude: excluded items in \[40, 40\] outside"):
            call(exclude=[(0, 40)])
    with pytest.raises(ValueError, match="k = 1025"):
        similar_items(t, [0], k=1025)
    with pytest.raises(ValueError, match=r"similar_items: items in \[-1, 3\] outside \[0, 40\)"):
        similar_items(t, [3, -1])
    wide = torch.zeros(2, 1025, device="cuda")
    with pytest.raises(ValueError, match=r"similar_items: d = 1025 outside \[1, 1024\]"):
        similar_items(wide)
    with pytest.raises(ValueError, match=r"evaluate_neighbours: d = 1025 outside \[1, 1024\]"):
        evaluate_neighbours(wide, [(0, 1)])
    with pytest.raises(ValueError, match="the held-out set is empty"):
        evaluate_neighbours(t, [])
    with pytest.raises(ValueError, match=r"heldout: items in \[0, 40\] outside \[0, 40\)"):
        evaluate_neighbours(t, [(0, 40)])
    with pytest.raises(ValueError, match="2 of 32 held-out pairs are also excluded"):
        evaluate_neighbours(t, edges, exclude=[(0, 1), (1, 0)])
    with pytest.raises(ValueError, match="ks="):
        evaluate_neighbours(t, edges, ks=())


def test_refusals_of_the_scorer_and_the_entries():
    t = dev(U.planted_table())
    with pytest.raises(ValueError, match="item_sim: the table must be a contiguous fp32 tensor on a GPU"):
        ItemSimScorer(t.cpu())
    with pytest.raises(ValueError, match="item_sim: the table must be a contiguous fp32 tensor on a GPU"):
        ItemSimScorer(t.t())
    with pytest.raises(ValueError, match="eps = 0.0 is not a positive finite number"):
        ItemSimScorer(t, eps=0.0)
    with pytest.raises(ValueError, match="metric='l1'"):
        ItemSimScorer(t, "l1")
    s = ItemSimScorer(t)
    q = dev(np.array([1, 2], dtype=np.int64))
    with pytest.raises(ValueError, match="queries must be a contiguous int64 tensor"):
        s.score(q.int())
    with pytest.raises(ValueError, match=r"out must be a contiguous fp32 tensor \[>= 2, >= 40\]"):
        s.score(q, out=torch.empty(2, 39, device="cuda"))
    # the entries themselves refuse what the surface would not pass on, before anything is launched
    lib = _lib.hip()
    out = torch.full((2, 40), SENTINEL, device="cuda")
    args = lambda **kw: [kw.get("table", t.data_ptr()), s.inv_norm.data_ptr(), q.data_ptr(), kw.get("n", 2), kw.get("n_items", 40), kw.get("d", 8),
                         out.data_ptr(), kw.get("stride", 40), _lib.stream()]
    for kw, text in ((dict(d=0), "d = 0 outside"), (dict(d=1025), "d = 1025 outside"), (dict(n=0), "n = 0 queries outside"),
                     (dict(n=(1 << 20) + 1), "queries outside"), (dict(n_items=0), "0 items outside"), (dict(stride=39), "row_stride = 39 below"),
                     (dict(table=0), "NULL buffer"), (dict(table=t.data_ptr() + 2), "misaligned buffer")):
        assert lib.pmgt_item_sim_score(*args(**kw)) == -2 and text in lib.pmgt_last_error().decode(), kw
    for a, text in (((t.data_ptr(), 40, 0, 1e-12, s.inv_norm.data_ptr(), _lib.stream()), "d = 0 outside"),
                    ((t.data_ptr(), 0, 8, 1e-12, s.inv_norm.data_ptr(), _lib.stream()), "0 items outside"),
                    ((t.data_ptr(), 40, 8, 0.0, s.inv_norm.data_ptr(), _lib.stream()), "not a positive finite number"),
                    ((t.data_ptr(), 40, 8, 1e-12, 0, _lib.stream()), "NULL buffer")):
        assert lib.pmgt_item_sim_norms(*a) == -2 and text in lib.pmgt_last_error().decode(), text
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
