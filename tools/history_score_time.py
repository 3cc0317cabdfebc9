"""What recommending from a user's history costs (A/B tool, not a test; tools/item_sim_time.py's protocol):

    python tools/history_score_time.py [--users 1024] [--rounds 5] [--calls 50] [--device-calls 5] [--host-calls 1] [--large-users 48]
                                       [--skip-large] [--out PATH]

Shapes: the item-sim tool's catalogues at d = 128 -- 7 252 items and 275 696 items --, 1 024 users a call, every user with a history of 5
and of 20 items.  Tables are standard normal, seeded; the histories are seeded draws without replacement, with two more items a user held
out.  Per shape, sides alternating in windows after one warm-up window of each side, in ONE process over the same tensors:
  fused / unfused / torch_profile / torch_profile_prenormalised        (both aggs for the first two)
        HistoryScorer.score (cosine; norms and CSR built once in the constructor) against
        - the unfused composition: ItemSimScorer.score on the flattened histories, then torch.segment_reduce over each user's rows (the
          general segment reduce, by the lengths of the lists).  It runs where its [users x length, I] fp32 score rows fit the 256 MiB
          workspace of the drivers; elsewhere the bytes it would need are reported instead;
        - torch's normalize(profile) @ normalize(t).T, profile = the mean of the normalised history rows, as it is written -- the table
          normalised on every call -- and on a normalised COPY made once.  It is the mean only, and its bits depend on the batch.
        One call a launch sequence, timed with device events.  With the fused time: the achieved TFLOP/s (2 * rows * I * d flops over the
        history rows; the f32 matrix peak is 157 TFLOP/s) and the bytes stored a call (4 n I).
  recommend_device / recommend_host    recommend_from_history(k=20), whole calls on a host clock around calls that end in a copy from the device
  evaluate_device / evaluate_host      evaluate_history on the held-out items, whole calls on a host clock
        (the large catalogue: the first --large-users users, the host side being minutes a call otherwise)
  odd_d   the fused kernel alone at 7 252 items and d = 130, histories of 5: d is no multiple of 4 there, so the kernel loads single floats
        and takes 256 VGPRs (one workgroup a CU) instead of 16-byte loads and 209
Prints one JSON line: per side the median, minimum, maximum and every window's microseconds per call, per pair the ratio of the medians
with its range.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from item_sim_time import PEAK_TFLOPS, alternate, device_window_us, host_window_us, ratio  # noqa: E402
from pmgt_amd.history import HistoryScorer, evaluate_history, recommend_from_history  # noqa: E402
from pmgt_amd.recommend import SCORE_WORKSPACE_BYTES  # noqa: E402
from pmgt_amd.similar import ItemSimScorer  # noqa: E402

K = 20


def draw(n_users, n_items, length, seed=0):
    """per user `length` history items and two held-out ones, all distinct -> (history pairs, held-out pairs) int64 [., 2]"""
    rng = np.random.default_rng(seed)
    picks = np.stack([rng.choice(n_items, size=length + 2, replace=False) for _ in range(n_users)]).astype(np.int64)
    owner = np.arange(n_users, dtype=np.int64)[:, None]
    hist = np.stack([np.broadcast_to(owner, (n_users, length)).ravel(), picks[:, :length].ravel()], axis=1)
    held = np.stack([np.broadcast_to(owner, (n_users, 2)).ravel(), picks[:, length:].ravel()], axis=1)
    return hist, held


def shape(n_items, d, n_users, length, whole_users, args, rounds):
    """every pair of sides on one catalogue and one history length -> dict"""
    gen = torch.Generator(device="cuda").manual_seed(29)
    table = torch.randn(n_items, d, generator=gen, device="cuda")
    hist, held = draw(n_users, n_items, length)
    users_d = torch.arange(n_users, device="cuda")
    res = {"items": n_items, "d": d, "users": n_users, "history": length}
    # 1. the kernel alone
    with torch.no_grad():
        fused = {agg: HistoryScorer(table, hist, n_users, agg, "cosine") for agg in ("mean", "max")}
        flat = torch.from_numpy(np.ascontiguousarray(fused["mean"].history[1]).astype(np.int64)).cuda()      # ascending per user
        out = fused["mean"].score(users_d)
        sides = {f"fused_{agg}": (lambda s=fused[agg]: s.score(users_d, out=out), args.calls) for agg in fused}
        unfused_bytes = 4 * n_users * length * n_items
        res["unfused_score_row_bytes"] = int(unfused_bytes)
        res["unfused_fits_workspace"] = bool(unfused_bytes <= SCORE_WORKSPACE_BYTES)
        if res["unfused_fits_workspace"]:
            sim = ItemSimScorer(table, "cosine")
            rows = torch.empty(n_users * length, n_items, dtype=torch.float32, device="cuda")
            lengths = torch.from_numpy(np.diff(fused["mean"].history[0])).cuda()
            red = [None]

            def unfused_mean():
                sim.score(flat, out=rows)
                red[0] = torch.segment_reduce(rows, "mean", lengths=lengths, axis=0, unsafe=True)

            def unfused_max():
                sim.score(flat, out=rows)
                red[0] = torch.segment_reduce(rows, "max", lengths=lengths, axis=0, unsafe=True)
            sides.update(unfused_mean=(unfused_mean, args.calls), unfused_max=(unfused_max, args.calls))
        tn = F.normalize(table, dim=1)
        ref = torch.empty_like(out)

        def profile():
            t = F.normalize(table, dim=1)
            torch.matmul(F.normalize(t[flat].view(n_users, length, d).mean(dim=1), dim=1), t.T, out=ref)

        def profile_pre():
            torch.matmul(F.normalize(tn[flat].view(n_users, length, d).mean(dim=1), dim=1), tn.T, out=ref)
        sides.update(torch_profile=(profile, args.calls), torch_profile_prenormalised=(profile_pre, args.calls))
        st = alternate(sides, rounds, device_window_us)
        if res["unfused_fits_workspace"]:
            unfused_mean()
            fused["mean"].score(users_d, out=out)
            res["max_abs_difference_fused_unfused_mean"] = float((out - red[0]).abs().max())      # (torch's sum has its own order: not the bits)
            del rows, red
    res.update(st)
    flops = 2.0 * n_users * length * n_items * d
    res["fused_mean_tflops"] = {k: round(flops / (st["fused_mean"][w] * 1e-6) / 1e12, 1) for k, w in (("median", "median"), ("low", "max"), ("high", "min"))}
    res["fused_mean_share_of_f32_matrix_peak"] = round(res["fused_mean_tflops"]["median"] / PEAK_TFLOPS, 3)
    res["bytes_stored_per_call"] = int(4 * n_users * n_items)
    if res["unfused_fits_workspace"]:
        res["unfused_over_fused_mean"] = ratio(st["unfused_mean"], st["fused_mean"])
        res["unfused_over_fused_max"] = ratio(st["unfused_max"], st["fused_max"])
    res["torch_profile_over_fused_mean"] = ratio(st["torch_profile"], st["fused_mean"])
    res["torch_profile_prenormalised_over_fused_mean"] = ratio(st["torch_profile_prenormalised"], st["fused_mean"])
    del out, ref, tn
    # 2. whole calls
    if whole_users < n_users:
        hist, held = hist[hist[:, 0] < whole_users], held[held[:, 0] < whole_users]
    res["whole_call_users"] = int(min(whole_users, n_users))
    host_table = table.cpu().numpy()
    dev = lambda: recommend_from_history(table, hist, k=K, impl="device")
    host = lambda: recommend_from_history(host_table, hist, k=K, impl="host")
    st = alternate({"recommend_device": (dev, args.device_calls), "recommend_host": (host, args.host_calls)}, rounds, host_window_us)
    res.update(st)
    res["recommend_host_over_device"] = ratio(st["recommend_host"], st["recommend_device"])
    dev = lambda: evaluate_history(table, hist, held, ks=(10, 20), impl="device")
    host = lambda: evaluate_history(host_table, hist, held, ks=(10, 20), impl="host")
    st = alternate({"evaluate_device": (dev, args.device_calls), "evaluate_host": (host, args.host_calls)}, rounds, host_window_us)
    res.update(st)
    res["evaluate_host_over_device"] = ratio(st["evaluate_host"], st["evaluate_device"])
    res["result_device"], res["result_host"] = dev(), host()
    return res


def odd_d(n_items, d, n_users, length, args):
    """the fused kernel alone at a d that is no multiple of 4 (single-float loads) -> dict"""
    gen = torch.Generator(device="cuda").manual_seed(29)
    table = torch.randn(n_items, d, generator=gen, device="cuda")
    hist, _ = draw(n_users, n_items, length)
    users_d = torch.arange(n_users, device="cuda")
    with torch.no_grad():
        fused = {agg: HistoryScorer(table, hist, n_users, agg, "cosine") for agg in ("mean", "max")}
        out = fused["mean"].score(users_d)
        st = alternate({f"fused_{agg}": (lambda s=fused[agg]: s.score(users_d, out=out), args.calls) for agg in fused}, args.rounds, device_window_us)
    res = {"items": n_items, "d": d, "users": n_users, "history": length}
    res.update(st)
    res["fused_mean_tflops"] = round(2.0 * n_users * length * n_items * d / (st["fused_mean"]["median"] * 1e-6) / 1e12, 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)            # launch sequences a window
    ap.add_argument("--device-calls", type=int, default=5)      # whole device calls a window
    ap.add_argument("--host-calls", type=int, default=1)        # whole host calls a window
    ap.add_argument("--large-users", type=int, default=48)      # users of the whole calls on the large catalogue
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("history_score_time.py needs a HIP device")
    res = {"metric": "history_score_time", "k": K, "f32_matrix_peak_tflops": PEAK_TFLOPS, "shapes": []}
    for length in (5, 20):
        res["shapes"].append(shape(7252, 128, args.users, length, args.users, args, args.rounds))
    res["odd_d"] = odd_d(7252, 130, args.users, 5, args)
    if not args.skip_large:
        args.calls, args.device_calls = max(1, args.calls // 10), max(1, args.device_calls // 5)
        for length in (5, 20):
            res["shapes"].append(shape(275696, 128, args.users, length, args.large_users, args, min(args.rounds, 3)))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
