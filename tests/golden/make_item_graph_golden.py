"""Regenerates tests/golden/item_graph.npz: a few interaction sets with the output of the reference's "Construct Product Graph" recipe as
tests/test_item_graph_cpu.py restates it (needs scipy and networkx; recorded with scipy 1.15 and networkx 3.4).

    python tests/golden/make_item_graph_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import test_item_graph_cpu as t  # noqa: E402
from pmgt_amd.item_graph import synthetic_interactions  # noqa: E402


def main():
    cases = [(*t.random_set(2), 3), (*t.random_set(9), 2), (*t.random_set(21), 1), (synthetic_interactions(120, 90, 2500, seed=1), 90, 3)]
    out = {"n_cases": np.int64(len(cases))}
    for k, (pairs, num_item, min_count) in enumerate(cases):
        g, c = t.recipe(pairs, num_item, min_count)
        edges = sorted((min(u, v), max(u, v)) for u, v in g.edges)
        assert edges
        out[f"pairs_{k}"] = pairs
        out[f"num_item_{k}"] = np.int64(num_item)
        out[f"min_count_{k}"] = np.int64(min_count)
        out[f"edges_{k}"] = np.array(edges, dtype=np.int64)
        out[f"counts_{k}"] = np.array([c[i, j] for i, j in edges], dtype=np.int64)
        out[f"weights_{k}"] = np.array([g.edges[i, j]["weight"] for i, j in edges], dtype=np.float64)
        out[f"items_{k}"] = np.array(sorted(g.nodes), dtype=np.int64)
    np.savez_compressed(os.path.join(HERE, "item_graph.npz"), **out)


if __name__ == "__main__":
    main()
