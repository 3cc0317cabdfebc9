"""What scoring a batch of users against the whole catalogue costs with the Deep & Cross Network, DcnScorer.score against DCN.forward on
pair rows (A/B tool, not a test; tools/ncf_model_score_time.py's protocol):

    python tools/dcn_score_time.py [--users 1024] [--rounds 5] [--calls 50] [--torch-calls 3] [--out PATH]

Two shapes, both with LayerNorm, 7 252 items, a batch of 1 024 users out of 50 000, each in ONE process over the same uploaded batch of ids:
  script     scripts/run_dcn.sh's: factor_num 16, 1 deep layer, 4 cross layers (E = 32; the VALU kernel)
  mfma       factor_num 64, 2 deep layers, 6 cross layers (E = 256; the MFMA tile at its widest)
and two sides:
  kernel     DcnScorer.score into a ready [users, items] buffer: the gather of the user rows, the Pu product, pmgt_dcn_score_rows over
             the batch and pmgt_dcn_score
  torch      recommend(impl="host")'s computation without its copies out: DCN.forward under torch.no_grad() in eval mode on chunks of 2^18
             (user, item) pair rows, written into the same kind of buffer
Both sides are warmed up by one window; then they alternate in windows of `calls` (torch: `torch-calls`) calls, each window timed with device
events on the launch stream.  Prints one JSON line: per shape and side the median, minimum, maximum and every window's microseconds per call,
and the ratio of the medians.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pmgt_amd.dcn import DCN  # noqa: E402
from pmgt_amd.recommend import DcnScorer  # noqa: E402

USERS, ITEMS = 50000, 7252
PAIR_CHUNK = 1 << 18                                         # dcn_host_scores' default
CASES = [("script", 16, 1, 4), ("mfma", 64, 2, 6)]


def window_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def make_model(factor, deep, cross):
    """A DCN with LayerNorm whose tensors are away from their init (embeddings O(1), gamma != 1, beta != 0, cross weights 0.3 / sqrt(D) so
    that 1 + s_c stays away from 0, as tests/dcn_util.random_dcn draws them)"""
    torch.manual_seed(0)
    model = DCN(USERS, ITEMS, factor, deep, cross, use_layer_norm=True).cuda().eval()
    D = 2 * (factor << deep)
    with torch.no_grad():
        for name, p in model.named_parameters():
            if name.endswith("embeddings.weight"):
                p.normal_(0.0, 1.0)
            elif name.startswith("cross_net") and name.endswith(".weight") and "layer_norm" not in name:
                p.normal_(0.0, 0.3 / D ** 0.5)
            elif p.dim() == 1:
                p.add_(0.3 * torch.randn_like(p))
    return model


def torch_rows(model, users, out):
    """dcn_host_scores without the copies out"""
    item_ids = torch.arange(ITEMS, device=users.device)
    per = max(1, PAIR_CHUNK // ITEMS)
    with torch.no_grad():
        for lo in range(0, len(users), per):
            u = users[lo: lo + per]
            m = len(u)
            out[lo: lo + m] = model((u[:, None].expand(m, ITEMS).reshape(-1), item_ids.repeat(m))).view(m, ITEMS)


def measure(factor, deep, cross, users, rounds, calls, torch_calls):
    model = make_model(factor, deep, cross)
    out_k, out_t = (torch.empty(len(users), ITEMS, device="cuda") for _ in range(2))
    scorer = DcnScorer(dict(model.state_dict()), None, model.layer_norm_eps)
    sides = {"kernel": (lambda: scorer.score(users, out=out_k), calls, []), "torch": (lambda: torch_rows(model, users, out_t), torch_calls, [])}
    for fn, n, _ in sides.values():                          # warm-up windows, not recorded
        window_us(fn, n)
    order = list(sides)
    for r in range(rounds):
        for name in (order if r % 2 == 0 else order[::-1]):
            fn, n, us = sides[name]
            us.append(window_us(fn, n))
    torch.cuda.synchronize()
    res = {"factor_num": factor, "deep_layers": deep, "cross_layers": cross, "layer_norm": True,
           "max_abs_difference_kernel_torch": float((out_k - out_t).abs().max()), "max_abs_score": float(out_t.abs().max())}
    for name, (_, n, us) in sides.items():
        res[f"{name}_us"] = {"median": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1),
                             "calls_per_window": n, "windows": [round(x, 1) for x in us]}
    k = res["kernel_us"]
    res["torch_over_kernel"] = {"median": round(res["torch_us"]["median"] / k["median"], 2),
                                "range": [round(res["torch_us"]["min"] / k["max"], 2), round(res["torch_us"]["max"] / k["min"], 2)]}
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
        raise SystemExit("dcn_score_time.py needs a HIP device")
    users = torch.from_numpy(np.random.default_rng(0).integers(0, USERS, size=args.users)).cuda()
    res = {"metric": "dcn_score_time", "batch_users": args.users, "users": USERS, "items": ITEMS, "cases": {}}
    for tag, factor, deep, cross in CASES:
        res["cases"][tag] = measure(factor, deep, cross, users, args.rounds, args.calls, args.torch_calls)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
