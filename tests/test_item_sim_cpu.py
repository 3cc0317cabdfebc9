"""The numpy side of the nearest-items feature: item_sim_host against a direct F.normalize product, the seeds of the rounded GPU case,
holdout_edges, edges_csr, and similar_items / evaluate_neighbours(impl="host") on a planted table, with their refusals.  No GPU."""
import os
import re

import numpy as np
import pytest

from pmgt_amd import _build, _lib
from pmgt_amd.catalogue_eval import catalogue_metrics_host, heldout_ranks_host
from pmgt_amd.graph import CSRGraph, synthetic_graph, synthetic_graph_regular
from pmgt_amd.recommend import topk_host
from pmgt_amd.similar import (edges_csr, evaluate_neighbours, holdout_edges, item_exclusion_csr, item_sim_host, similar_items)
from tests import item_sim_util as U


def undirected(graph):
    """the set of undirected edges {(a, b): weight} of a CSRGraph, a < b node ids; asserts that both directions carry the weight"""
    src = np.repeat(np.arange(graph.n_nodes + 2), np.diff(graph.indptr))
    both = {(int(a), int(b)): float(w) for a, b, w in zip(src, graph.indices, graph.weights)}
    assert len(both) == len(src) and all(both[(b, a)] == w for (a, b), w in both.items())
    return {e: w for e, w in both.items() if e[0] < e[1]}


def test_item_sim_host_is_the_normalized_product():
    import torch
    import torch.nn.functional as F
    t = U.normal_table(33, 3)[:50]
    q = np.array([7, 0, 49, 7])
    want = (F.normalize(torch.from_numpy(t).double(), dim=1)[q] @ F.normalize(torch.from_numpy(t).double(), dim=1).T).numpy()
    got = item_sim_host(t, q, "cosine", dtype=np.float64)
    assert got.dtype == np.float64 and got.shape == (4, 50) and np.abs(got - want).max() <= 8 * 2.0 ** -52
    got32 = item_sim_host(t, q)
    assert got32.dtype == np.float32 and np.abs(got32 - want).max() <= 64 * 2.0 ** -24
    dot = item_sim_host(t, q, "dot", dtype=np.float64)
    assert np.abs(dot - (t.astype(np.float64)[q] @ t.astype(np.float64).T)).max() <= 1e-12
    # every item by default; symmetric bit for bit in the scalings' order; F.normalize's clamp on a zero row
    z = t.copy()
    z[5] = 0
    full = item_sim_host(z)
    assert full.shape == (50, 50) and (full[5] == 0).all() and (full[:, 5] == 0).all()
    scaled = item_sim_host(np.diag(np.float32([2.0 ** -70, 2.0])), eps=1e-12, dtype=np.float64)
    assert scaled[0, 0] == (2.0 ** -140 * (1 / 1e-12)) * (1 / 1e-12) and scaled[1, 1] == 1.0 and scaled[0, 1] == 0.0
    # a NaN stays in its row and column
    z[9, 2] = np.nan
    bad = np.isnan(item_sim_host(z))
    want_bad = np.zeros((50, 50), bool)
    want_bad[9] = want_bad[:, 9] = True
    assert np.array_equal(bad, want_bad)
    with pytest.raises(ValueError, match="metric='l2'"):
        item_sim_host(t, q, "l2")
    with pytest.raises(ValueError, match=r"item_sim_host: queries in \[50, 50\] outside \[0, 50\)"):
        item_sim_host(t, [50])


@pytest.mark.parametrize("d", U.DS)
def test_the_seeds_of_the_rounded_case_are_decided_by_the_yardstick(d):
    assert U.SEEDS[d] >= U.FIRST_SEED
    for seed in range(U.FIRST_SEED, U.SEEDS[d]):
        assert U.second_worst(d, seed) > U.C_BOUND, seed     # the FIRST such seed
    assert U.second_worst(d, U.SEEDS[d]) <= U.C_BOUND


def test_query_lists_are_unordered_with_one_id_twice():
    for n_items in U.ITEMS:
        q = U.queries_of(n_items)
        assert len(q) == U.NS[-1] and q.min() >= 0 and q.max() < n_items and q[3] == q[0]
        assert n_items == 1 or (np.diff(q) < 0).any()


def test_holdout_edges_regular_graph():
    g = synthetic_graph_regular(200, 800, seed=1)
    before = undirected(g)
    train, held = holdout_edges(g, 0.1, seed=0)
    assert isinstance(train, CSRGraph) and train.n_nodes == 200
    train.validate()                                         # no isolated node
    assert held.dtype == np.int64 and held.shape == (80, 2) and (held[:, 0] < held[:, 1]).all()      # round(0.1 * 800), degree 8 allows it
    again_train, again_held = holdout_edges(g, 0.1, seed=0)
    assert np.array_equal(held, again_held) and np.array_equal(train.indptr, again_train.indptr)
    assert np.array_equal(train.indices, again_train.indices) and np.array_equal(train.weights, again_train.weights)
    other = holdout_edges(g, 0.1, seed=1)[1]
    assert not np.array_equal(held, other)
    kept = undirected(train)
    out = {(int(a) + 2, int(b) + 2) for a, b in held}
    assert len(out) == 80 and not out & set(kept) and out | set(kept) == set(before)
    assert all(before[e] == w for e, w in kept.items())      # the weights travel with their edges
    # the remaining edges stay in their original adjacency order
    for v in range(2, 202):
        old = [int(u) for u in g.neighbors(v) if (min(u, v), max(u, v)) in kept]
        assert old == train.neighbors(v).tolist()
    assert len(holdout_edges(g, 0.0)[1]) == 0 and np.array_equal(holdout_edges(g, 0.0)[0].indices, g.indices)


def test_holdout_edges_keeps_every_node_connected():
    # a ring plus a few chords: most nodes have degree 2, so far fewer than the asked edges can leave
    g = synthetic_graph(60, 70, seed=2)
    train, held = holdout_edges(g, 0.9, seed=3)
    train.validate()
    assert 0 < len(held) < round(0.9 * 70)
    kept = undirected(train)
    assert len(kept) + len(held) == 70
    # the walk, restated: no further edge of the permutation's order could have left
    deg = np.diff(train.indptr)
    assert all(deg[a] == 1 or deg[b] == 1 for a, b in kept)
    with pytest.raises(ValueError, match="fraction = 1.0 outside"):
        holdout_edges(g, 1.0)
    with pytest.raises(ValueError, match="expected a CSRGraph"):
        holdout_edges(np.zeros((3, 2)), 0.1)


def test_holdout_edges_composes_with_item_graph():
    from pmgt_amd.item_graph import item_graph_host, synthetic_interactions
    ig = item_graph_host(synthetic_interactions(80, 60, 1500, seed=0), 60, min_count=2)
    n = ig.graph.n_nodes
    train, held = holdout_edges(ig.graph, 0.2, seed=0)
    train.validate()
    assert len(held) >= 1 and train.n_nodes == n and len(train.indices) + 2 * len(held) == len(ig.graph.indices)
    # rows of the table are the graph's nodes (node id - 2); the training graph is the exclusion list
    t = np.random.default_rng(0).standard_normal((n, 6)).astype(np.float32)
    res = evaluate_neighbours(t, held, exclude=train, impl="host")
    assert res["items"] == len(np.unique(held)) and res["pairs"] == 2 * len(held)


def test_edges_csr_is_symmetric_and_drops_duplicates():
    indptr, items = edges_csr([(0, 3), (3, 0), (2, 1), (0, 3), (4, 0)], 5)
    assert indptr.dtype == np.int64 and items.dtype == np.int32
    assert indptr.tolist() == [0, 2, 3, 4, 5, 6] and items.tolist() == [3, 4, 2, 1, 0, 0]
    indptr, items = edges_csr([(0, 3), (0, 3), (2, 1)], 5, symmetric=False)
    assert indptr.tolist() == [0, 1, 1, 2, 2, 2] and items.tolist() == [3, 1]
    assert edges_csr([], 4)[0].tolist() == [0] * 5 and len(edges_csr(None, 4)[1]) == 0
    with pytest.raises(ValueError, match=r"heldout: items in \[0, 5\] outside \[0, 5\)"):
        edges_csr([(0, 5)], 5, who="heldout")
    with pytest.raises(ValueError, match=r"edges: expected \(item, item\) integer pairs"):
        edges_csr(np.zeros((2, 3), dtype=np.int64), 5)
    # the exclusion CSR over item ids: pairs, a ready CSR or a graph, plus the diagonal
    g = synthetic_graph(6, 8, seed=0)
    indptr, items = item_exclusion_csr(g, 6, True)
    for v in range(6):
        assert items[indptr[v]: indptr[v + 1]].tolist() == sorted(set((g.neighbors(v + 2) - 2).tolist()) | {v})
    plain = item_exclusion_csr(g, 6, False)
    assert len(plain[1]) == len(g.indices) and len(items) == len(g.indices) + 6
    again = item_exclusion_csr(plain, 6, True)
    assert np.array_equal(again[0], indptr) and np.array_equal(again[1], items)
    assert item_exclusion_csr(None, 3, True)[1].tolist() == [0, 1, 2] and len(item_exclusion_csr(None, 3, False)[1]) == 0
    with pytest.raises(ValueError, match="the graph has 6 nodes, the table 7 rows"):
        item_exclusion_csr(g, 7, True)


def test_similar_items_host_on_the_planted_table():
    t = U.planted_table()
    found, scores = similar_items(t, k=6, impl="host")
    assert found.shape == (40, 6) and found.dtype == np.int64 and scores.dtype == np.float32
    for i in range(40):
        c = i // 5
        assert sorted(found[i, :4].tolist()) == [j for j in range(5 * c, 5 * c + 5) if j != i]      # the cluster first, never the item itself
        assert i not in found[i] and (np.diff(scores[i]) <= 0).all() and scores[i, 3] > 0.9 > 0.5 > scores[i, 4]
    # the yardstick pieces, put together by hand
    indptr, excl = item_exclusion_csr(None, 40, True)
    q = np.array([17, 3, 17])
    want = topk_host(item_sim_host(t, q), 6, indptr, excl, q)
    got = similar_items(t, q, k=6, impl="host")
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    cut = similar_items(t, q, k=6, impl="host", batch_items=2)      # (numpy's product may round otherwise in another batch: the ids only)
    assert np.array_equal(cut[0], want[0]) and np.abs(cut[1] - want[1]).max() <= 2.0 ** -22
    # self kept: the item is its own nearest (cosine 1); an exclusion list; fewer than k eligible items pad with -1 / -inf
    assert (similar_items(t, q, k=1, exclude_self=False, impl="host")[0][:, 0] == q).all()
    gone = [(17, j) for j in range(15, 20)]
    assert not set(similar_items(t, [17], k=20, exclude=gone, impl="host")[0][0].tolist()) & set(range(15, 20))
    few, few_scores = similar_items(t[:3], [0], k=5, impl="host")
    assert few[0, 2:].tolist() == [-1, -1, -1] and (few_scores[0, 2:] == -np.inf).all() and sorted(few[0, :2].tolist()) == [1, 2]
    # dot product: another order than the cosine when the norms differ
    big = np.array(t)
    big[39] *= 50
    assert similar_items(big, [0], k=1, metric="dot", impl="host")[0][0, 0] != similar_items(big, [0], k=1, impl="host")[0][0, 0]
    import torch
    assert np.array_equal(similar_items(torch.from_numpy(np.array(t)), q, k=6, impl="host")[0], want[0].astype(np.int64))


def test_evaluate_neighbours_host_on_the_planted_table():
    t, edges = U.planted_table(), U.planted_edges()
    res, rec = evaluate_neighbours(t, edges, ks=(4, 10), impl="host", per_item=True)
    assert list(res) == ["n4", "n10", "r4", "r10", "hr4", "hr10", "mrr", "items", "pairs"]
    assert res["items"] == 32 and res["pairs"] == 32 and res["r10"] == 1.0 and res["r4"] == 1.0 and res["hr4"] == 1.0
    assert rec["ranks"].min() >= 1 and rec["ranks"].max() <= 4      # within the cluster, the item itself excluded
    assert np.array_equal(rec["items"], np.unique(edges)) and (rec["n_pos"] == 1).all()
    # the pieces by hand, in one batch and in several
    h = edges_csr(edges, 40, True)
    e = item_exclusion_csr(None, 40, True)
    q = rec["items"]
    ranks, flags = heldout_ranks_host(item_sim_host(t, q), q, h, e)
    m = catalogue_metrics_host(ranks, h[0], (4, 10))
    assert not flags.any() and np.array_equal(rec["ranks"], ranks) and np.array_equal(rec["indptr"], h[0]) and np.array_equal(rec["heldout"], h[1])
    for k in (4, 10):
        assert np.array_equal(rec["ndcg"][k], m["ndcg"][k]) and res[f"n{k}"] == m["sums"]["ndcg"][k] / 32
    assert np.array_equal(rec["rr"], m["rr"]) and res["mrr"] == m["sums"]["rr"] / 32
    assert evaluate_neighbours(t, edges, ks=(4, 10), impl="host", batch_items=5) == res
    assert evaluate_neighbours(t, np.concatenate([edges, edges[:3, ::-1]]), ks=(4, 10), impl="host") == res      # duplicates are dropped
    # with the cluster's other edges excluded (a training graph) the held-out neighbour is first or second
    train = [(5 * c + a, 5 * c + b) for c in range(8) for a, b in ((0, 2), (1, 3))]
    res2, rec2 = evaluate_neighbours(t, edges, exclude=train + [(b, a) for a, b in train], ks=(4, 10), impl="host", per_item=True)
    assert (rec2["ranks"] <= rec["ranks"]).all() and (rec2["ranks"] < rec["ranks"]).any() and res2["mrr"] > res["mrr"]
    # without the self exclusion the item itself takes the first place
    assert evaluate_neighbours(t, edges, ks=(1,), exclude_self=False, impl="host")["hr1"] == 0.0


def test_refusals():
    t, edges = U.planted_table(), U.planted_edges()
    for call in (lambda **kw: similar_items(t, [0], **kw), lambda **kw: evaluate_neighbours(t, edges, **kw)):
        with pytest.raises(ValueError, match="impl='cpu'"):
            call(impl="cpu")
        with pytest.raises(ValueError, match="metric='l2'"):
            call(metric="l2", impl="host")
        with pytest.raises(ValueError, match="batch_items = 0"):
            call(batch_items=0, impl="host")
        with pytest.raises(ValueError, match=r"exclude: excluded items in \[-1, -1\] outside"):
            call(exclude=[(0, -1)], impl="host")
    wide = np.zeros((2, 1025), dtype=np.float32)
    with pytest.raises(ValueError, match=r"similar_items: d = 1025 outside \[1, 1024\]"):
        similar_items(wide, impl="host")
    with pytest.raises(ValueError, match=r"evaluate_neighbours: d = 1025 outside \[1, 1024\]"):
        evaluate_neighbours(wide, [(0, 1)], impl="host")
    with pytest.raises(ValueError, match="similar_items: the table must be an fp32 array"):
        similar_items(t.astype(np.float64), impl="host")
    for k in (0, 1025, 2.5, True):
        with pytest.raises(ValueError, match="k = "):
            similar_items(t, [0], k=k, impl="host")
    with pytest.raises(ValueError, match=r"similar_items: items in \[40, 40\] outside \[0, 40\)"):
        similar_items(t, [40], impl="host")
    with pytest.raises(ValueError, match=r"items .* must be \[Q >= 1\]"):
        similar_items(t, [], impl="host")
    with pytest.raises(ValueError, match="ks="):
        evaluate_neighbours(t, edges, ks=(20, 10), impl="host")
    with pytest.raises(ValueError, match="the held-out set is empty"):
        evaluate_neighbours(t, [], impl="host")
    with pytest.raises(ValueError, match=r"heldout: items in \[0, 40\] outside \[0, 40\)"):
        evaluate_neighbours(t, [(0, 40)], impl="host")
    with pytest.raises(ValueError, match="2 of 32 held-out pairs are also excluded"):
        evaluate_neighbours(t, edges, exclude=[(0, 1), (1, 0), (0, 2)], impl="host")
    with pytest.raises(ValueError, match="1 of 1 held-out pairs are also excluded"):
        evaluate_neighbours(t, [(3, 3)], impl="host")        # a self edge meets the self exclusion
    # a NaN: eligible for every query but those that exclude the item, named by their number
    bad = np.array(t)
    bad[4, 1] = np.nan
    with pytest.raises(ValueError, match="similar_items: 2 of 3 items have a NaN score among their eligible items"):
        similar_items(bad, [0, 1, 2], exclude=[(1, 4)], impl="host")
    similar_items(bad, [0, 1], exclude=[(0, 4), (1, 4)], impl="host")      # excluded for all: no error
    with pytest.raises(ValueError, match="evaluate_neighbours: 3 of 4 items have a NaN score among their eligible items"):
        evaluate_neighbours(bad, [(0, 1), (2, 3)], exclude=[(2, 4)], impl="host")


def test_the_entries_are_declared_bound_and_built():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "pmgt_capi.h")).read()
    for sym in ("pmgt_item_sim_norms", "pmgt_item_sim_score"):
        assert re.search(r"\b" + sym + r"\(", hdr) and sym in _lib.HIP_SYMBOLS, sym
    assert any(p.endswith(os.path.join("ops", "item_sim.hip")) for p in _build.OPS_SOURCES)
    assert "#define PMGT_ITEM_SIM_MAX_D 1024" in hdr and _lib.ITEM_SIM_MAX_D == 1024
    import pmgt_amd
    for name in ("item_sim_host", "ItemSimScorer", "similar_items", "evaluate_neighbours", "holdout_edges", "edges_csr"):
        assert name in pmgt_amd.__all__ and hasattr(pmgt_amd, name)
    assert callable(pmgt_amd.recommend) and callable(pmgt_amd.similar_items)
    from pmgt_amd.similar import ItemSimScorer      # noqa: F401  (the submodule stays reachable)
