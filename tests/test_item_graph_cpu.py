"""item_graph_host against the reference's "Construct Product Graph" recipe (notebooks/PMGT.ipynb cell 20), restated here with scipy and
networkx, and against recorded fixtures; the surface of build_item_graph that needs no GPU."""
import os
import re

import numpy as np
import pytest

import pmgt_amd
from pmgt_amd import _build, _lib, item_graph as ig
from pmgt_amd.graph import CSRGraph
from pmgt_amd.item_graph import ItemGraph, build_item_graph, item_graph_host, synthetic_interactions

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "item_graph.npz")
N_RANDOM = 58


def random_set(seed):
    """3 to 60 items, 3 to 40 users, 20 to 900 pairs with duplicates; catalogue indices beyond the used ones stay without interaction"""
    rs = np.random.RandomState(1000 + seed)
    n_item, n_user, n_pairs = rs.randint(3, 61), rs.randint(3, 41), rs.randint(20, 901)
    users = rs.choice(10 ** 6, size=n_user, replace=False)               # sparse ids
    skew = rs.random_sample(n_item) ** 2 + 0.02
    pairs = np.stack([users[rs.randint(0, n_user, n_pairs)], rs.choice(n_item, size=n_pairs, p=skew / skew.sum())], 1).astype(np.int64)
    return pairs, int(n_item + rs.randint(0, 3))


def recipe(pairs, num_item, min_count):
    """The notebook's cell in its own order: binary item-by-user matrix, sparse A A^T, diagonal removed, entries >= min_count into an
    nx.Graph, then the weight of every edge from the count and the two degrees.  -> nx.Graph over catalogue indices"""
    sp = pytest.importorskip("scipy.sparse")
    nx = pytest.importorskip("networkx")
    users = np.unique(pairs[:, 0])
    a = sp.dok_matrix((num_item, len(users)), dtype=np.int32)
    for u, i in zip(np.searchsorted(users, pairs[:, 0]), pairs[:, 1]):
        a[int(i), int(u)] = 1
    a = a.tocsr()
    c = (a @ a.T).tocsr()
    c.setdiag(0)
    c.eliminate_zeros()
    g = nx.Graph()
    for i in range(c.shape[0]):
        row = c.getrow(i)
        for j, r in zip(row.indices, row.data):
            if r >= min_count:
                g.add_edge(int(i), int(j), weight=r)
    for u, v, w in list(g.edges.data("weight")):
        g.edges[u, v]["weight"] = (np.log(w) + 1) / (np.log(np.sqrt(g.degree[u] * g.degree[v])) + 1)
    return g, c


def upper_of(res: ItemGraph):
    """-> (edges [E, 2] in catalogue indices with i < j, row-major; counts; weights) of the stored CSR"""
    g = res.graph
    row = np.repeat(np.arange(g.n_nodes + 2, dtype=np.int64), np.diff(g.indptr))
    up = row < g.indices
    return np.stack([res.items[row[up] - 2], res.items[g.indices[up] - 2]], 1), res.counts[up], g.weights[up]


def check_against_recipe(res: ItemGraph, g, c):
    assert sorted(g.nodes) == res.items.tolist()                          # the same node set
    edges, counts, weights = upper_of(res)
    assert sorted((min(u, v), max(u, v)) for u, v in g.edges) == [tuple(e) for e in edges.tolist()]      # the same edge set, ours row-major
    for (i, j), cnt, w in zip(edges.tolist(), counts.tolist(), weights):
        assert c[i, j] == cnt
        assert np.float64(g.edges[i, j]["weight"]).view(np.uint64) == np.float64(w).view(np.uint64), (i, j)      # all 64 bits
    check_structure(res)


def check_structure(res: ItemGraph):
    g = res.graph
    g.validate()
    for v in range(2, g.n_nodes + 2):
        assert (np.diff(g.neighbors(v)) > 0).all()                       # strictly ascending
    assert g.degree(0) == 0 and g.degree(1) == 0
    edges, counts, weights = upper_of(res)
    ref = CSRGraph.from_edge_list(g.n_nodes, res.node_of_item[edges], weights)
    assert np.array_equal(ref.indptr, g.indptr) and np.array_equal(ref.indices, g.indices)
    assert np.array_equal(ref.weights.view(np.uint64), g.weights.view(np.uint64))
    # node_of_item and items are inverse to each other
    assert np.array_equal(res.node_of_item[res.items], np.arange(2, g.n_nodes + 2))
    assert (np.delete(res.node_of_item, res.items) == -1).all() and (np.diff(res.items) > 0).all()
    # the counts are symmetric: the entry (a, b) equals the entry (b, a)
    row = np.repeat(np.arange(g.n_nodes + 2, dtype=np.int64), np.diff(g.indptr))
    sym = {(a, b): k for a, b, k in zip(row.tolist(), g.indices.tolist(), res.counts.tolist())}
    assert all(sym[(b, a)] == k for (a, b), k in sym.items())


def same_bits(x: ItemGraph, y: ItemGraph):
    assert np.array_equal(x.graph.indptr, y.graph.indptr) and np.array_equal(x.graph.indices, y.graph.indices)
    assert np.array_equal(x.counts, y.counts) and np.array_equal(x.items, y.items) and np.array_equal(x.node_of_item, y.node_of_item)
    assert np.array_equal(x.graph.weights.view(np.uint64), y.graph.weights.view(np.uint64))
    assert x.graph.n_nodes == y.graph.n_nodes


@pytest.mark.parametrize("min_count", [1, 2, 3])
def test_host_equals_the_recipe_on_random_sets(min_count):
    done = 0
    for seed in range(N_RANDOM):
        pairs, num_item = random_set(seed)
        g, c = recipe(pairs, num_item, min_count)
        if g.number_of_edges() == 0:
            with pytest.raises(ValueError, match="no edge"):
                item_graph_host(pairs, num_item, min_count)
            continue
        check_against_recipe(item_graph_host(pairs, num_item, min_count), g, c)
        done += 1
    assert done >= 50


def test_host_equals_the_recorded_fixtures():
    """inputs and the recipe's outputs as recorded with scipy 1.15 / networkx 3.4: does not hang on what is installed"""
    gold = np.load(GOLDEN)
    n = int(gold["n_cases"])
    assert n >= 3
    for k in range(n):
        res = item_graph_host(gold[f"pairs_{k}"], int(gold[f"num_item_{k}"]), int(gold[f"min_count_{k}"]))
        edges, counts, weights = upper_of(res)
        assert np.array_equal(edges, gold[f"edges_{k}"]) and np.array_equal(counts, gold[f"counts_{k}"])
        assert np.array_equal(weights.view(np.uint64), gold[f"weights_{k}"].view(np.uint64))
        assert np.array_equal(res.items, gold[f"items_{k}"])
        check_structure(res)


def test_sorted_key_form_equals_the_dense_form(monkeypatch):
    pairs, num_item = random_set(7)
    big = synthetic_interactions(300, 500, 6000, seed=3)
    dense = [item_graph_host(pairs, num_item, 2), item_graph_host(big, 500, 2)]
    monkeypatch.setattr(ig, "DENSE_MAX_ITEMS", 0)
    monkeypatch.setattr(ig, "HOST_CHUNK", 1000)                          # many steps, several merges
    same_bits(item_graph_host(pairs, num_item, 2), dense[0])
    same_bits(item_graph_host(big, 500, 2), dense[1])


def test_row_order_and_duplicates_do_not_matter():
    pairs, num_item = random_set(11)
    want = item_graph_host(pairs, num_item, 2)
    rs = np.random.RandomState(0)
    same_bits(item_graph_host(pairs[rs.permutation(len(pairs))], num_item, 2), want)
    distinct = np.unique(pairs, axis=0)
    assert len(distinct) < len(pairs)
    same_bits(item_graph_host(distinct, num_item, 2), want)
    same_bits(item_graph_host(np.concatenate([pairs, pairs[::3], pairs]), num_item, 2), want)      # duplicates count once
    import torch
    same_bits(item_graph_host(torch.from_numpy(pairs), num_item, 2), want)
    same_bits(build_item_graph(pairs, num_item, 2, impl="host"), want)


def test_an_item_below_min_count_is_no_node():
    # items 0, 1, 2 share users 0..2; item 3 shares two users with item 0; item 4 has one user; item 5 has none
    pairs = np.array([(u, i) for i in (0, 1, 2) for u in (0, 1, 2)] + [(0, 3), (1, 3), (7, 3), (2, 4)], dtype=np.int64)
    res = item_graph_host(pairs, 6, 3)
    assert res.items.tolist() == [0, 1, 2] and res.node_of_item.tolist() == [2, 3, 4, -1, -1, -1]
    assert res.counts.tolist() == [3] * 6 and res.graph.indices.tolist() == [3, 4, 2, 4, 2, 3]
    assert np.array_equal(res.graph.weights, np.full(6, (np.log(3) + 1) / (np.log(np.sqrt(4)) + 1)))
    assert item_graph_host(pairs, 6, 2).items.tolist() == [0, 1, 2, 3]
    assert item_graph_host(pairs, 6, 1).items.tolist() == [0, 1, 2, 3, 4]


def test_filter_pairs_keeps_the_rows_whose_item_is_a_node():
    import torch
    pairs, num_item = random_set(5)
    res = item_graph_host(pairs, num_item, 3)
    later = np.stack([np.arange(200), np.random.RandomState(1).randint(0, num_item, 200)], 1).astype(np.int64)
    want = later[np.isin(later[:, 1], res.items)]
    assert 0 < len(want) < len(later)
    assert np.array_equal(res.filter_pairs(later), want)
    assert np.array_equal(res.filter_pairs(torch.from_numpy(later)).numpy(), want)


def test_the_sampler_takes_the_graph():
    from pmgt_amd.datasets import MODE_TRAIN, MCNSampler
    res = item_graph_host(synthetic_interactions(80, 60, 1500, seed=2), 60, 3)
    smp = MCNSampler(res.graph, 7)
    smp.seed(0)
    n = min(8, res.graph.n_nodes)
    tgt = smp.batch(np.arange(2, 2 + n), MODE_TRAIN)[0]
    ids = tgt["node_ids"].numpy()
    assert ids.shape[0] == n and ids.max() <= res.graph.n_nodes + 1 and (ids[:, 0] == np.arange(2, 2 + n)).all()


def test_to_networkx_has_the_recipes_edges_and_weights():
    pytest.importorskip("networkx")
    pairs, num_item = random_set(3)
    g, _ = recipe(pairs, num_item, 2)
    mine = item_graph_host(pairs, num_item, 2).to_networkx()
    assert sorted(mine.nodes) == sorted(g.nodes)
    assert {frozenset(e) for e in mine.edges} == {frozenset(e) for e in g.edges}
    for u, v, w in g.edges.data("weight"):
        assert isinstance(mine.edges[u, v]["weight"], float) and mine.edges[u, v]["weight"] == float(w)


def test_the_generator_is_seeded_and_skewed():
    a, b = synthetic_interactions(500, 300, 20000, seed=4), synthetic_interactions(500, 300, 20000, seed=4)
    assert np.array_equal(a, b) and a.dtype == np.int64 and a.shape == (20000, 2)
    assert not np.array_equal(a, synthetic_interactions(500, 300, 20000, seed=5))
    assert a[:, 0].min() >= 0 and a[:, 0].max() < 500 and a[:, 1].min() >= 0 and a[:, 1].max() < 300
    pop = np.sort(np.bincount(a[:, 1], minlength=300))[::-1]
    assert pop[0] > 8 * pop[-1] and pop[:30].sum() > 0.25 * len(a)      # Zipf-like: a head and a long tail
    assert len(np.unique(a, axis=0)) < len(a)                            # rows repeat


@pytest.mark.parametrize("impl", ["host", "device"])
def test_refusals(impl, monkeypatch):
    """every refusal is raised before anything is launched: impl="device" gets as far as these checks without a GPU"""
    ok = np.array([[0, 0], [0, 1], [1, 0], [1, 1]], dtype=np.int64)
    call = lambda pairs=ok, num_item=4, min_count=1: build_item_graph(pairs, num_item, min_count, impl=impl)
    for bad in (ok.astype(np.int32), ok.ravel(), np.zeros((4, 3), dtype=np.int64), ok.tolist()):
        with pytest.raises(ValueError, match=r"int64.*\[P, 2\]"):
            call(pairs=bad)
    with pytest.raises(ValueError, match="negative"):
        call(pairs=np.array([[0, 0], [-1, 1]], dtype=np.int64))
    with pytest.raises(ValueError, match="negative"):
        call(pairs=np.array([[0, -2], [1, 1]], dtype=np.int64))
    with pytest.raises(ValueError, match="item 4 outside"):
        call(pairs=np.array([[0, 4], [1, 1]], dtype=np.int64))
    with pytest.raises(ValueError, match="above 2\\^31 - 2"):
        call(num_item=2 ** 31 - 1)
    with pytest.raises(ValueError, match="not below 2\\^31"):
        call(pairs=np.array([[2 ** 31, 0], [1, 1]], dtype=np.int64))
    for bad in (0, -3, 1.5, True):
        with pytest.raises(ValueError, match="min_count"):
            call(min_count=bad)
    for bad in (0, -1, 2.0):
        with pytest.raises(ValueError, match="num_item"):
            call(num_item=bad)
    with pytest.raises(ValueError, match="impl"):
        build_item_graph(ok, 4, 1, impl="scipy")
    if impl == "host":                                                   # (the device path counts the distinct pairs on the device)
        monkeypatch.setattr(ig, "MAX_PAIRS", 3)
        with pytest.raises(ValueError, match="4 distinct pairs"):
            call()
        monkeypatch.undo()
        with pytest.raises(ValueError, match=r"min_count = 3 users \(the largest count seen is 2\)"):
            call(min_count=3)
        with pytest.raises(ValueError, match="largest count seen is 0"):
            call(pairs=np.array([[0, 0], [1, 1], [2, 2]], dtype=np.int64))      # all singletons
        with pytest.raises(ValueError, match="largest count seen is 0"):
            call(pairs=np.zeros((0, 2), dtype=np.int64))
        assert call(min_count=2).items.tolist() == [0, 1]


def test_the_entries_are_registered():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "pmgt_capi.h")).read()
    for sym in ("pmgt_item_graph_count", "pmgt_item_graph_fill", "pmgt_item_graph_default_slots"):
        assert re.search(r"\b" + sym + r"\(", hdr) and sym in _lib.HIP_SYMBOLS, sym
    assert hdr.index("pmgt_rank_heldout_reduce(") < hdr.index("pmgt_item_graph_count(")
    assert any(p.endswith(os.path.join("ops", "item_graph.hip")) for p in _build.OPS_SOURCES)
    assert f"#define PMGT_ITEM_GRAPH_MIN_SLOTS {_lib.ITEM_GRAPH_MIN_SLOTS}\n" in hdr
    assert f"#define PMGT_ITEM_GRAPH_MAX_SLOTS {_lib.ITEM_GRAPH_MAX_SLOTS}\n" in hdr
    for name in ("ItemGraph", "build_item_graph", "item_graph_host", "synthetic_interactions"):
        assert getattr(pmgt_amd, name) is getattr(ig, name) and name in pmgt_amd.__all__
