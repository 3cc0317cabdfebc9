"""What building the item graph from interactions costs (A/B tool, not a test; tools/catalogue_eval_time.py's protocol):

    python tools/item_graph_time.py [--shapes a,b] [--rounds 5] [--host-b] [--out PATH]

Two generated shapes (synthetic_interactions, seed 0, min_count 3):
  a   the notebook's printout: 48 270 items, 507 775 interactions (70 000 users)
  b   10^6 items, 2 x 10^7 interactions (2 x 10^6 users): the scale bench.py's c4 trains on
Per shape two pairs of sides, each pair alternating in windows after one warm-up window of each side, in ONE process over the same inputs:
  build_device / host_recipe   build_item_graph(impl="device") end to end from host pairs (upload, dedupe, CSR images, both passes, the copy
                               back, the weights) against the recipe's host path: scipy's sparse product and threshold when scipy is
                               importable (the matrix from the deduplicated pairs, A A^T, diagonal removed, entries >= 3 -- without the
                               notebook's Python loops and without networkx, which only favours the host), else item_graph_host; host clock
  count_kernels / fill_kernels the two entries alone on ready CSRs (two launches each), device events
At shape b the host side runs once with --host-b and is skipped with a note without it; the device result is then checked on 1 000 sampled
rows against a per-row host count.  Prints one JSON line per shape as it finishes and one with everything at the end: per side the median, minimum, maximum and every window's milliseconds per call,
per pair the ratio of the medians with its range, the nodes and edges that came out, the rows that took each path.  Needs a GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pmgt_amd.item_graph import ItemGraphKernels, build_item_graph, device_csrs, item_graph_host, synthetic_interactions  # noqa: E402

SHAPES = {"a": dict(users=70000, items=48270, pairs=507775), "b": dict(users=2000000, items=1000000, pairs=20000000)}
MIN_COUNT = 3


def device_window_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def host_window_ms(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / n


def alternate(sides, rounds, window):
    """sides: {name: (fn, calls a window)}; one warm-up window each, then `rounds` alternating windows -> {name: stats}"""
    ms = {name: [] for name in sides}
    for fn, n in sides.values():
        window(fn, n)
    order = list(sides)
    for r in range(rounds):
        for name in (order if r % 2 == 0 else order[::-1]):
            fn, n = sides[name]
            ms[name].append(window(fn, n))
    return {name: {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3),
                   "calls_per_window": sides[name][1], "windows": [round(x, 3) for x in v]} for name, v in ms.items()}


def ratio(slow, fast):
    return {"median": round(slow["median"] / fast["median"], 2), "range": [round(slow["min"] / fast["max"], 2), round(slow["max"] / fast["min"], 2)]}


def scipy_recipe(pairs, num_item):
    """the recipe's host path up to the thresholded upper triangle -> number of edges"""
    import scipy.sparse as sp
    users, col = np.unique(pairs[:, 0], return_inverse=True)
    a = sp.csr_matrix((np.ones(len(pairs), dtype=np.int32), (pairs[:, 1], col)), shape=(num_item, len(users)))
    a.data[:] = 1                                            # binary: duplicates were summed
    c = (a @ a.T).tocsr()
    c.setdiag(0)
    c.eliminate_zeros()
    return int(np.count_nonzero(c.data >= MIN_COUNT)) // 2


def check_sampled_rows(res, pairs, num_item, n_rows=1000):
    """per-row host count of `n_rows` sampled catalogue rows against the device result -> rows compared"""
    keys = np.unique(pairs[:, 0] * np.int64(num_item) + pairs[:, 1])
    users, user = np.unique(keys // num_item, return_inverse=True)
    item = keys % num_item
    user_ptr = np.concatenate([[0], np.cumsum(np.bincount(user, minlength=len(users)))])
    order = np.argsort(item, kind="stable")
    item_ptr = np.concatenate([[0], np.cumsum(np.bincount(item, minlength=num_item))])
    rs = np.random.RandomState(0)
    rows = np.unique(np.concatenate([rs.randint(0, num_item, n_rows - 20), np.argsort(np.diff(item_ptr))[-20:]]))      # with the longest rows
    g = res.graph
    for i in rows:
        us = user[order[item_ptr[i]: item_ptr[i + 1]]]
        js = np.concatenate([item[user_ptr[u]: user_ptr[u + 1]] for u in us]) if len(us) else np.zeros(0, dtype=np.int64)
        j, c = np.unique(js[js != i], return_counts=True)
        keep = c >= MIN_COUNT
        node = res.node_of_item[i]
        if not keep.any():
            assert node == -1, i
            continue
        assert np.array_equal(res.items[g.neighbors(node) - 2], j[keep]), i
        assert np.array_equal(res.counts[g.indptr[node]: g.indptr[node + 1]], c[keep]), i
    return int(len(rows))


def measure(name, rounds, host_b):
    s = SHAPES[name]
    pairs = synthetic_interactions(s["users"], s["items"], s["pairs"], seed=0)
    n = s["items"]
    out = dict(s)
    res = build_item_graph(pairs, n, MIN_COUNT, impl="device")
    out.update(nodes=int(res.graph.n_nodes), edges=int(len(res.counts) // 2), fallback_rows=int(len(res.fallback_items)))
    # the kernels alone
    keys = torch.unique(torch.from_numpy(pairs[:, 0] * np.int64(n) + pairs[:, 1]).cuda())
    csrs = device_csrs(keys, n)
    k = ItemGraphKernels(csrs, n, MIN_COUNT)
    deg = k.count() & 0x7FFFFFFF
    row_ptr = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    torch.cumsum(deg, 0, dtype=torch.int64, out=row_ptr[1:])
    total = int(row_ptr[-1].item())
    node = torch.where(deg > 0, torch.cumsum(deg > 0, 0) + 1, -1).to(torch.int32)
    idx, cnt = torch.empty(total, dtype=torch.int32, device="cuda"), torch.empty(total, dtype=torch.int32, device="cuda")
    work = csrs["work"]
    out.update(distinct_pairs=int(keys.numel()), expansions=int(work.sum().item()), wave_rows=int(((work > 0) & (work <= k.slots // 4 * 3)).sum().item()),
               workgroup_rows=int((work > k.slots // 4 * 3).sum().item()), slots=k.slots, scratch_rows=k.scratch_rows)
    calls = 5 if name == "a" else 1
    st = alternate({"count_kernels": (k.count, calls), "fill_kernels": (lambda: k.fill(row_ptr, node, total, idx, cnt), calls)}, rounds,
                   device_window_ms)
    out.update(st)
    for side in ("count_kernels", "fill_kernels"):
        out[side + "_expansions_per_ns"] = round(out["expansions"] / (st[side]["median"] * 1e6), 2)
    # end to end against the host
    dev = lambda: build_item_graph(pairs, n, MIN_COUNT, impl="device")
    try:
        import scipy.sparse  # noqa: F401
        host, out["host_side"] = (lambda: scipy_recipe(pairs, n)), "scipy product and threshold"
    except ImportError:
        host, out["host_side"] = (lambda: item_graph_host(pairs, n, MIN_COUNT)), "item_graph_host"
    if name == "a":
        st = alternate({"build_device": (dev, 3), "host_recipe": (host, 1)}, rounds, host_window_ms)
        out.update(st)
        out["host_over_device"] = ratio(st["host_recipe"], st["build_device"])
        if "scipy" in out["host_side"]:
            assert scipy_recipe(pairs, n) == out["edges"]
    else:
        out.update(alternate({"build_device": (dev, 1)}, rounds, host_window_ms))
        if host_b:
            t0 = time.perf_counter()
            edges = host()
            out["host_recipe"] = {"once_ms": round((time.perf_counter() - t0) * 1e3, 1)}
            out["host_over_device"] = {"once": round(out["host_recipe"]["once_ms"] / out["build_device"]["median"], 2)}
            if "scipy" in out["host_side"]:
                assert edges == out["edges"]
        else:
            out["host_recipe"] = "skipped: the product at this shape takes minutes and tens of GB on the host (pass --host-b to run it once)"
        out["sampled_rows_checked"] = check_sampled_rows(res, pairs, n)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="a,b")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--host-b", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("item_graph_time.py needs a HIP device")
    res = {"metric": "item_graph_time", "min_count": MIN_COUNT, "unit": "ms"}
    for name in args.shapes.split(","):
        res[name] = measure(name, args.rounds, args.host_b)
        print(json.dumps({name: res[name]}), flush=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
