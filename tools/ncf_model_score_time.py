"""What scoring a batch of users against the whole catalogue costs with the stand-alone NCF class, NcfModelScorer.score against its
yardsticks (A/B tool, not a test; tools/ncf_model_step_time.py's protocol):

    python tools/ncf_model_score_time.py [--users 1024] [--rounds 5] [--calls 50] [--torch-calls 3] [--out PATH]

The reference's shape: factor_num 64, 2 layers (d = 128), 7 252 items, a batch of 1 024 users out of 50 000.  Two cases, kind NeuMF-end with
LayerNorm and kind GMF, each in ONE process over the same uploaded batch of user ids:
  kernel     NcfModelScorer.score into a ready [users, items] buffer: the Pu product and pmgt_ncf_model_score
  torch      host_scores' computation without its copies out: model.head in eval mode on chunks of 2^18 (user, item) pair rows gathered
             from the table, written into the same kind of buffer
  no_ln      (the LayerNorm case only) NcfScorer.score, the existing kernel WITHOUT LayerNorm, on a head of the same shape: what the
             statistics cost
All sides are warmed up by one window; then they alternate in windows of `calls` (torch: `torch-calls`) calls, each window timed with device
events on the launch stream.  Prints one JSON line: per case and side the median, minimum, maximum and every window's microseconds per call,
and the ratios of the medians.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pmgt_amd.ncf import NCF  # noqa: E402
from pmgt_amd.recommend import NcfModelScorer, NcfScorer  # noqa: E402

FACTOR, LAYERS, USERS, ITEMS = 64, 2, 50000, 7252
PAIR_CHUNK = 1 << 18                                         # host_scores' default
CASES = [("neumf_ln", "NeuMF-end", True), ("gmf", "GMF", False)]


def window_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def make_model(kind, ln):
    """An NCF of the reference's shape whose tensors are away from their init (embeddings O(1), gamma != 1, beta != 0): the init's 0.01
    embeddings would leave every LayerNorm row at the scale of eps"""
    torch.manual_seed(0)
    model = NCF(USERS, ITEMS, FACTOR, LAYERS, use_layer_norm=ln, model=kind).cuda().eval()
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.startswith("embed_"):
                p.normal_(0.0, 1.0 if ln or kind == "GMF" else 0.5)
            elif p.dim() == 1:
                p.add_(0.3 * torch.randn_like(p))
    return model


def torch_rows(model, table, users, out):
    """host_scores without the copies out"""
    n_items = ITEMS
    item_ids = torch.arange(n_items, device=users.device)
    per = max(1, PAIR_CHUNK // n_items)
    with torch.no_grad():
        for lo in range(0, len(users), per):
            u = users[lo: lo + per]
            m = len(u)
            out[lo: lo + m] = model.head(u[:, None].expand(m, n_items).reshape(-1), item_ids.repeat(m), table.repeat(m, 1)).view(m, n_items)


def measure(kind, ln, users, rounds, calls, torch_calls):
    model = make_model(kind, ln)
    sd = model.state_dict()
    out_k, out_t = (torch.empty(len(users), ITEMS, device="cuda") for _ in range(2))
    scorer = NcfModelScorer(sd, None, kind, model.layer_norm_eps)
    table = torch.empty(ITEMS, 0, device="cuda") if kind == "GMF" else model.embed_item_MLP.weight.detach()
    sides = {"kernel": (lambda: scorer.score(users, out=out_k), calls, []), "torch": (lambda: torch_rows(model, table, users, out_t), torch_calls, [])}
    if ln:                                                   # the same tensors read as a PMGT_NCF head without LayerNorm
        head = {"mlp_user_embeddings.weight": sd["embed_user_MLP.weight"], "gmf_user_embeddings.weight": sd["embed_user_GMF.weight"],
                "gmf_item_embeddings.weight": sd["embed_item_GMF.weight"], "predict_layer.weight": sd["predict_layer.weight"],
                "predict_layer.bias": sd["predict_layer.bias"]}
        for i in range(LAYERS):
            head[f"mlp_layers.{i}.linear.weight"], head[f"mlp_layers.{i}.linear.bias"] = sd[f"MLP_layers.{4 * i}.weight"], sd[f"MLP_layers.{4 * i}.bias"]
        plain = NcfScorer(head, table)
        out_p = torch.empty(len(users), ITEMS, device="cuda")
        sides["no_ln"] = (lambda: plain.score(users, out=out_p), calls, [])
    for fn, n, _ in sides.values():                          # warm-up windows, not recorded
        window_us(fn, n)
    order = list(sides)
    for r in range(rounds):
        for name in (order if r % 2 == 0 else order[::-1]):
            fn, n, us = sides[name]
            us.append(window_us(fn, n))
    torch.cuda.synchronize()
    res = {"kind": kind, "layer_norm": ln, "max_abs_difference_kernel_torch": float((out_k - out_t).abs().max()),
           "max_abs_score": float(out_t.abs().max())}
    for name, (_, n, us) in sides.items():
        res[f"{name}_us"] = {"median": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1),
                             "calls_per_window": n, "windows": [round(x, 1) for x in us]}
    k = res["kernel_us"]
    res["torch_over_kernel"] = {"median": round(res["torch_us"]["median"] / k["median"], 2),
                                "range": [round(res["torch_us"]["min"] / k["max"], 2), round(res["torch_us"]["max"] / k["min"], 2)]}
    if ln:
        p = res["no_ln_us"]
        res["kernel_over_no_ln"] = {"median": round(k["median"] / p["median"], 3), "range": [round(k["min"] / p["max"], 3), round(k["max"] / p["min"], 3)]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--torch-calls", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ncf_model_score_time.py needs a HIP device")
    users = torch.from_numpy(np.random.default_rng(0).integers(0, USERS, size=args.users)).cuda()
    res = {"metric": "ncf_model_score_time", "factor_num": FACTOR, "num_layers": LAYERS, "batch_users": args.users, "users": USERS, "items": ITEMS,
           "cases": {}}
    for tag, kind, ln in CASES:
        res["cases"][tag] = measure(kind, ln, users, args.rounds, args.calls, args.torch_calls)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
