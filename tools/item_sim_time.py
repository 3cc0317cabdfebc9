"""What the nearest items from the embeddings cost (A/B tool, not a test; tools/catalogue_eval_time.py's protocol):

    python tools/item_sim_time.py [--queries 1024] [--rounds 5] [--calls 200] [--device-calls 10] [--host-calls 1] [--skip-large] [--out PATH]

Shapes: the reference script's catalogue, 7 252 items at d = 128 and d = 256 with 1 024 queries a call, and the item-graph tool's larger
catalogue, 275 696 items at d = 128 with batch_items at its default (the 256 MiB of score rows: 243 queries a call).  Tables are standard
normal, seeded.  Per shape, pairs of sides alternating in windows after one warm-up window of each side, in ONE process over the same
tensors:
  score_kernel / torch_product / torch_prenormalised
        ItemSimScorer.score (cosine; the norms were computed once in the constructor) against torch's
        normalize(t)[q] @ normalize(t).T as it is written -- the table normalised on every call -- and against tn[q] @ tn.T on a normalised
        COPY made once, the copy this feature does not keep; one call a launch, timed with device events.  With the kernel's time: the
        achieved TFLOP/s (2 n I d flops; the f32 matrix peak is 157 TFLOP/s) and the bytes stored a call (4 n I).
  similar_device / similar_host        similar_items(k=20) on the same queries, whole calls on a host clock around calls that end in a
        copy from the device
  neighbours_device / neighbours_host  evaluate_neighbours on a holdout_edges split of a seeded synthetic graph, the training graph
        excluded, whole calls on a host clock (the large catalogue: the first edges of the split that give one batch of queries)
Prints one JSON line: per side the median, minimum, maximum and every window's microseconds per call, per pair the ratio of the medians
with its range.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pmgt_amd.graph import synthetic_graph, synthetic_graph_regular  # noqa: E402
from pmgt_amd.recommend import default_batch_users  # noqa: E402
from pmgt_amd.similar import ItemSimScorer, evaluate_neighbours, holdout_edges, similar_items  # noqa: E402

PEAK_TFLOPS = 157.3
K = 20


def device_window_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def host_window_us(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / n


def alternate(sides, rounds, window):
    """sides: {name: (fn, calls a window)}; one warm-up window each, then `rounds` alternating windows -> {name: stats}"""
    us = {name: [] for name in sides}
    for fn, n in sides.values():
        window(fn, n)
    order = list(sides)
    for r in range(rounds):
        for name in (order if r % 2 == 0 else order[::-1]):
            fn, n = sides[name]
            us[name].append(window(fn, n))
    return {name: {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1),
                   "calls_per_window": sides[name][1], "windows": [round(x, 1) for x in v]} for name, v in us.items()}


def ratio(slow, fast):
    return {"median": round(slow["median"] / fast["median"], 2), "range": [round(slow["min"] / fast["max"], 2), round(slow["max"] / fast["min"], 2)]}


def shape(n_items, d, n_queries, graph, fraction, max_edges, args, rounds):
    """every pair of sides on one catalogue -> dict"""
    gen = torch.Generator(device="cuda").manual_seed(29)
    table = torch.randn(n_items, d, generator=gen, device="cuda")
    queries = np.sort(np.random.default_rng(0).choice(n_items, size=n_queries, replace=False)).astype(np.int64)
    q_d = torch.from_numpy(queries).cuda()
    res = {"items": n_items, "d": d, "queries": n_queries}
    # 1. the kernel alone
    with torch.no_grad():
        scorer = ItemSimScorer(table, "cosine")
        out = scorer.score(q_d)
        tn = F.normalize(table, dim=1)
        ref = torch.empty_like(out)
        st = alternate({"score_kernel": (lambda: scorer.score(q_d, out=out), args.calls),
                        "torch_product": (lambda: torch.matmul(F.normalize(table, dim=1)[q_d], F.normalize(table, dim=1).T, out=ref), args.calls),
                        "torch_prenormalised": (lambda: torch.matmul(tn[q_d], tn.T, out=ref), args.calls)}, rounds, device_window_us)
        res["max_abs_difference_from_torch"] = float((out - ref).abs().max())
    res.update(st)
    flops = 2.0 * n_queries * n_items * d
    res["score_kernel_tflops"] = {k: round(flops / (st["score_kernel"][w] * 1e-6) / 1e12, 1) for k, w in (("median", "median"), ("low", "max"), ("high", "min"))}
    res["score_kernel_share_of_f32_matrix_peak"] = round(res["score_kernel_tflops"]["median"] / PEAK_TFLOPS, 3)
    res["bytes_stored_per_call"] = int(4 * n_queries * n_items)
    res["torch_product_over_kernel"] = ratio(st["torch_product"], st["score_kernel"])
    res["torch_prenormalised_over_kernel"] = ratio(st["torch_prenormalised"], st["score_kernel"])
    del out, ref, tn
    # 2. similar_items, whole calls
    host_table = table.cpu().numpy()
    dev = lambda: similar_items(table, queries, k=K, impl="device")
    host = lambda: similar_items(host_table, queries, k=K, impl="host")
    st = alternate({"similar_device": (dev, args.device_calls), "similar_host": (host, args.host_calls)}, rounds, host_window_us)
    res.update(st)
    res["similar_host_over_device"] = ratio(st["similar_host"], st["similar_device"])
    # 3. evaluate_neighbours, whole calls
    train, held = holdout_edges(graph, fraction, seed=0)
    held = held[:max_edges] if max_edges else held
    dev = lambda: evaluate_neighbours(table, held, exclude=train, ks=(10, 20), impl="device")
    host = lambda: evaluate_neighbours(host_table, held, exclude=train, ks=(10, 20), impl="host")
    st = alternate({"neighbours_device": (dev, args.device_calls), "neighbours_host": (host, args.host_calls)}, rounds, host_window_us)
    res.update(st)
    res["neighbours_host_over_device"] = ratio(st["neighbours_host"], st["neighbours_device"])
    res["heldout_edges"], res["result_device"], res["result_host"] = int(len(held)), dev(), host()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)           # kernel launches a window
    ap.add_argument("--device-calls", type=int, default=10)     # whole device calls a window
    ap.add_argument("--host-calls", type=int, default=1)        # whole host calls a window
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("item_sim_time.py needs a HIP device")
    res = {"metric": "item_sim_time", "k": K, "f32_matrix_peak_tflops": PEAK_TFLOPS, "shapes": []}
    small = synthetic_graph(7252, 5 * 7252, seed=0)
    for d in (128, 256):
        res["shapes"].append(shape(7252, d, args.queries, small, 0.02, 0, args, args.rounds))
    if not args.skip_large:
        n_items = 275696
        batch = default_batch_users(n_items, n_items)        # batch_items at its default: 243 queries a call
        args.calls, args.device_calls = max(1, args.calls // 10), max(1, args.device_calls // 5)
        res["shapes"].append(shape(n_items, 128, batch, synthetic_graph_regular(n_items, 4 * n_items, seed=0), 0.001, batch // 2, args,
                                   min(args.rounds, 3)))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
