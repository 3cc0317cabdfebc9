"""What evaluating on the whole catalogue costs (A/B tool, not a test; tools/dcn_score_time.py's protocol):

    python tools/catalogue_eval_time.py [--users 1024] [--rounds 5] [--calls 1000] [--eval-calls 20] [--host-calls 3] [--out PATH]

The reference script's shape: the stand-alone NCF class, NeuMF-end with LayerNorm, factor_num 64, 2 layers, 7 252 items, 1 024 evaluated users
out of 50 000 in one call, each with 20 excluded (training) items and 5 held-out ones.  Three pairs of sides, each pair alternating in
windows after one warm-up window of each side, in ONE process over the same inputs:
  rank_kernel / topk_kernel      HeldoutRanks.rank against TopkRows.select(k=20) on the same ready score rows [1 024, 7 252] with the same
                                 exclusion CSR: one launch each, `calls` launches a window, timed with device events; with them, for
                                 scale, score_kernels: NcfModelScorer.score producing those rows (the gather, the Pu product, the fused head)
                                 (a window relaunches on the same 29.7 MB of rows, which stay in the 256 MiB last-level cache: the two
                                 kernels are compared like for like, neither figure is a rate of reads from HBM)
  catalogue_device / catalogue_host      evaluate_catalogue(impl="device") against impl="host", whole calls (the CSRs built, the table
                                 projected, every copy) on a host clock around calls that end in a copy from the device
  catalogue_device / sampled_device      evaluate_catalogue(impl="device") against evaluate_ranking(metrics="device") on the same users with
                                 their held-out items and negatives up to 100 candidates (the reference's protocol; the candidate lists are
                                 built once, outside the timing)
Prints one JSON line: per side the median, minimum, maximum and every window's microseconds per call, and per pair the ratio of the medians
with its range.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pmgt_amd.catalogue_eval import HeldoutRanks, evaluate_catalogue, heldout_csr  # noqa: E402
from pmgt_amd.datasets import ranking_candidates  # noqa: E402
from pmgt_amd.evaluation import evaluate_ranking  # noqa: E402
from pmgt_amd.ncf import NCF  # noqa: E402
from pmgt_amd.recommend import NcfModelScorer, TopkRows, exclusion_csr  # noqa: E402

FACTOR, LAYERS, USERS, ITEMS = 64, 2, 50000, 7252
N_EXCLUDED, N_HELDOUT, NUM_NG, K = 20, 5, 100, 20


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


def make_model():
    """tools/ncf_model_score_time.py's model: tensors away from their init (embeddings O(1), gamma != 1, beta != 0)"""
    torch.manual_seed(0)
    model = NCF(USERS, ITEMS, FACTOR, LAYERS, use_layer_norm=True, model="NeuMF-end").cuda().eval()
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.startswith("embed_"):
                p.normal_(0.0, 1.0)
            elif p.dim() == 1:
                p.add_(0.3 * torch.randn_like(p))
    return model


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=1000)          # kernel launches a window: tens of milliseconds
    ap.add_argument("--eval-calls", type=int, default=20)      # whole device evaluations a window
    ap.add_argument("--host-calls", type=int, default=3)       # whole host evaluations a window
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("catalogue_eval_time.py needs a HIP device")
    rng = np.random.default_rng(0)
    users = np.sort(rng.choice(USERS, size=args.users, replace=False)).astype(np.int64)
    held, excl = [], []
    for u in users:
        drawn = rng.choice(ITEMS, size=N_EXCLUDED + N_HELDOUT, replace=False)
        held += [(int(u), int(i)) for i in drawn[:N_HELDOUT]]
        excl += [(int(u), int(i)) for i in drawn[N_HELDOUT:]]
    h_csr, e_csr = heldout_csr(held, USERS, ITEMS), exclusion_csr(excl, USERS, ITEMS)
    model = make_model()
    res = {"metric": "catalogue_eval_time", "evaluated_users": args.users, "users": USERS, "items": ITEMS, "factor_num": FACTOR,
           "num_layers": LAYERS, "kind": "NeuMF-end", "layer_norm": True, "heldout_per_user": N_HELDOUT, "excluded_per_user": N_EXCLUDED}
    # 1. the kernels alone, on the same score rows
    with torch.no_grad():
        scorer = NcfModelScorer(model.state_dict(), None, model.model, model.layer_norm_eps)
        users_d = torch.from_numpy(users).cuda()
        scores = scorer.score(users_d)
        ranker = HeldoutRanks("cuda", ITEMS, *h_csr, USERS, *e_csr)
        picker = TopkRows("cuda", args.users, ITEMS, K, *e_csr, USERS)
        flags = torch.zeros(args.users, dtype=torch.int32, device="cuda")
        out = picker.select(scores, users_d)
        again = torch.empty_like(scores)
        st = alternate({"rank_kernel": (lambda: ranker.rank(scores, users_d, flags), args.calls),
                        "topk_kernel": (lambda: picker.select(scores, users_d, out=out), args.calls),
                        "score_kernels": (lambda: scorer.score(users_d, out=again), max(1, args.calls // 10))}, args.rounds, device_window_us)
    res.update(st)
    res["score_row_bytes"] = int(scores.numel() * 4)
    res["rank_kernel_cache_resident_row_gb_per_s"] = round(scores.numel() * 4 / st["rank_kernel"]["median"] / 1e3, 1)
    res["topk_over_rank"] = ratio(st["topk_kernel"], st["rank_kernel"])
    # 2. whole calls: the device path against the host path
    dev = lambda: evaluate_catalogue(model, None, h_csr, exclude=e_csr, ks=(10, 20), impl="device")
    host = lambda: evaluate_catalogue(model, None, h_csr, exclude=e_csr, ks=(10, 20), impl="host")
    st = alternate({"catalogue_device": (dev, args.eval_calls), "catalogue_host": (host, args.host_calls)}, args.rounds, host_window_us)
    res.update(st)
    res["host_over_device"] = ratio(st["catalogue_host"], st["catalogue_device"])
    res["result_device"], res["result_host"] = dev(), host()
    # 3. whole calls: the whole catalogue against the reference's sampled candidates, both on the device
    cands = ranking_candidates(held, USERS, ITEMS, NUM_NG, seed=3)
    sampled = lambda: evaluate_ranking(model, None, *cands, ks=(10, 20), batch_users=256, metrics="device")
    st = alternate({"catalogue_device_again": (dev, args.eval_calls), "sampled_device": (sampled, args.eval_calls)}, args.rounds, host_window_us)
    res.update(st)
    res["catalogue_over_sampled"] = ratio(st["catalogue_device_again"], st["sampled_device"])
    res["result_sampled"] = sampled()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
