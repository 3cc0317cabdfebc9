"""What the truncated item-kNN costs (A/B tool, not a test; tools/item_sim_time.py's protocol):

    python tools/item_knn_time.py [--users 1024] [--rounds 5] [--calls 50] [--device-calls 5] [--host-calls 1] [--large-users 48]
                                  [--skip-small] [--skip-large] [--out PATH]

Shapes: the history tool's catalogues at d = 128 -- 7 252 items with 1 024 users a call and 275 696 items with --large-users users a call --,
every user with a history of 5 and of 20 items, the index built ONCE per catalogue at m = 256 and read at m = 16, 64 and 256 through
truncated().  Tables are standard normal, seeded; the histories are the history tool's seeded draws, two more items a user held out.  Per
shape, sides alternating in windows after one warm-up window of each side, in ONE process over the same tensors:
  knn_m16 / knn_m64 / knn_m256 / history_mean / torch_sparse_m64
        ItemKnnScorer.score (pmgt_knn_score; index, CSR and weights uploaded once) against
        - HistoryScorer(agg="mean").score on the same users: the dense kernel, |H| I d matrix work a user;
        - a torch sparse restatement at m = 64: the history matrix [users, I] (CSR, ones) times the index matrix [I, I] (CSR, m entries a
          row) by torch.sparse.mm, then to_dense().  Its sums have their own order: not the bits.  If torch refuses the product in CSR the
          COO layout is tried, and what was run (or the refusal) is reported.
        knn_weighted_m64 is the m = 64 side with a weight per entry.  One call a launch sequence, timed with device events.  With each knn
        time: the bytes stored a call (4 n I) over the time, next to the 6.29 TB/s a float4 copy reaches on this chip.
  build            build_item_knn(m = 256) end to end, whole calls on a host clock (a call ends in the copy of the NaN flags)
  recommend_device / recommend_host    recommend_item_knn(k = 20, m = 64) on the built index, whole calls on a host clock
  evaluate_device / evaluate_host      evaluate_item_knn(m = 64) on the held-out items, whole calls on a host clock
Prints one JSON line: per side the median, minimum, maximum and every window's microseconds per call, per pair the ratio of the medians
with its range.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from history_score_time import draw  # noqa: E402
from item_sim_time import alternate, device_window_us, host_window_us, ratio  # noqa: E402
from pmgt_amd.history import HistoryScorer  # noqa: E402
from pmgt_amd.item_knn import ItemKnnScorer, build_item_knn, evaluate_item_knn, recommend_item_knn  # noqa: E402

K = 20
MS = (16, 64, 256)
COPY_TBS = 6.29                                              # a float4 copy on this chip (README)


def sparse_sides(index, m, hist_csr, n_users, n_items):
    """the history matrix and the index matrix of the torch restatement -> ({layout: (H, S)}, the errors of the layouts torch refused)"""
    indptr, items = hist_csr
    rows = torch.from_numpy(np.repeat(np.arange(n_users, dtype=np.int64), np.diff(indptr))).cuda()
    H = torch.sparse_coo_tensor(torch.stack([rows, torch.from_numpy(items.astype(np.int64)).cuda()]),
                                torch.ones(len(items), device="cuda"), (n_users, n_items)).coalesce()
    nbr, sim = index.nbr[:, :m].reshape(-1).long(), index.sim[:, :m].reshape(-1)
    owner = torch.arange(n_items, device="cuda").repeat_interleave(m)
    live = nbr >= 0
    S = torch.sparse_coo_tensor(torch.stack([owner[live], nbr[live]]), sim[live], (n_items, n_items)).coalesce()
    made, errors = {}, {}
    for layout, conv in (("csr", lambda x: x.to_sparse_csr()), ("coo", lambda x: x)):
        try:
            h, s = conv(H), conv(S)
            torch.sparse.mm(h, s).to_dense()
            torch.cuda.synchronize()
            made[layout] = (h, s)
            break
        except RuntimeError as e:
            errors[layout] = str(e).splitlines()[0][:200]
    return made, errors


def shape(table, index, n_users, length, whole_users, args, rounds):
    """every pair of sides on one catalogue and one history length -> dict"""
    n_items, d = (int(v) for v in table.shape)
    hist, held = draw(n_users, n_items, length)
    users_d = torch.arange(n_users, device="cuda")
    res = {"items": n_items, "d": d, "users": n_users, "history": length}
    with torch.no_grad():
        knn = {m: ItemKnnScorer(index, hist, n_users, m=m) for m in MS}
        weights = np.random.default_rng(1).uniform(0.5, 5.0, size=len(hist)).astype(np.float32)
        weighted = ItemKnnScorer(index, hist, n_users, weights, m=64)
        dense = HistoryScorer(table, hist, n_users, "mean", "cosine")
        out = knn[64].score(users_d)
        ref = dense.score(users_d)
        sides = {f"knn_m{m}": (lambda s=knn[m]: s.score(users_d, out=out), args.calls) for m in MS}
        sides["knn_weighted_m64"] = (lambda: weighted.score(users_d, out=out), args.calls)
        sides["history_mean"] = (lambda: dense.score(users_d, out=ref), args.calls)
        made, errors = sparse_sides(index, 64, knn[64].history, n_users, n_items)
        res["torch_sparse_refused"] = errors
        for layout, (h, s) in made.items():
            res["torch_sparse_layout"] = layout
            keep = [None]

            def sparse(h=h, s=s):
                keep[0] = torch.sparse.mm(h, s).to_dense()
            sides["torch_sparse_m64"] = (sparse, args.calls)
        st = alternate(sides, rounds, device_window_us)
        if made:
            knn[64].score(users_d, out=out)
            sparse()
            res["max_abs_difference_knn_torch_sparse"] = float((out - keep[0]).abs().max())
            del keep
    res.update(st)
    stored = 4 * n_users * n_items
    res["bytes_stored_per_call"] = int(stored)
    for m in MS:
        t = st[f"knn_m{m}"]
        res[f"knn_m{m}_store_tbs"] = {k: round(stored / (t[w] * 1e-6) / 1e12, 2) for k, w in (("median", "median"), ("low", "max"), ("high", "min"))}
        res[f"knn_m{m}_share_of_copy_rate"] = round(res[f"knn_m{m}_store_tbs"]["median"] / COPY_TBS, 3)
        res[f"history_mean_over_knn_m{m}"] = ratio(st["history_mean"], t)
    res["knn_weighted_over_knn_m64"] = ratio(st["knn_weighted_m64"], st["knn_m64"])
    if made:
        res["torch_sparse_over_knn_m64"] = ratio(st["torch_sparse_m64"], st["knn_m64"])
    del out, ref, made
    # whole calls
    if whole_users < n_users:
        hist, held = hist[hist[:, 0] < whole_users], held[held[:, 0] < whole_users]
    res["whole_call_users"] = int(min(whole_users, n_users))
    host_index = index.truncated(64).host()
    dev = lambda: recommend_item_knn(index, hist, k=K, m=64, impl="device")
    host = lambda: recommend_item_knn(host_index, hist, k=K, impl="host")
    st = alternate({"recommend_device": (dev, args.device_calls), "recommend_host": (host, args.host_calls)}, rounds, host_window_us)
    res.update(st)
    res["recommend_host_over_device"] = ratio(st["recommend_host"], st["recommend_device"])
    dev = lambda: evaluate_item_knn(index, hist, held, ks=(10, 20), m=64, impl="device")
    host = lambda: evaluate_item_knn(host_index, hist, held, ks=(10, 20), impl="host")
    st = alternate({"evaluate_device": (dev, args.device_calls), "evaluate_host": (host, args.host_calls)}, rounds, host_window_us)
    res.update(st)
    res["evaluate_host_over_device"] = ratio(st["evaluate_host"], st["evaluate_device"])
    res["result_device"], res["result_host"] = dev(), host()
    return res


def catalogue(n_items, d, n_users, whole_users, args, rounds, build_rounds):
    """the index built (and its build timed: one call a window), then both history lengths -> (build dict, [shape dicts])"""
    gen = torch.Generator(device="cuda").manual_seed(29)
    table = torch.randn(n_items, d, generator=gen, device="cuda")
    keep = [None]

    def build():
        keep[0] = build_item_knn(table, MS[-1])
    st = alternate({"build": (build, 1)}, build_rounds, host_window_us)
    built = {"items": n_items, "d": d, "m": MS[-1], "index_bytes": int(8 * n_items * MS[-1])}
    built.update(st)
    return built, [shape(table, keep[0], n_users, length, whole_users, args, rounds) for length in (5, 20)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)            # launch sequences a window
    ap.add_argument("--device-calls", type=int, default=5)      # whole device calls a window
    ap.add_argument("--host-calls", type=int, default=1)        # whole host calls a window
    ap.add_argument("--large-users", type=int, default=48)      # users a call on the large catalogue
    ap.add_argument("--skip-small", action="store_true")
    ap.add_argument("--skip-large", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("item_knn_time.py needs a HIP device")
    res = {"metric": "item_knn_time", "k": K, "ms": list(MS), "float4_copy_tbs": COPY_TBS, "builds": [], "shapes": []}
    if not args.skip_small:
        built, shapes = catalogue(7252, 128, args.users, args.users, args, args.rounds, args.rounds)
        res["builds"].append(built)
        res["shapes"] += shapes
    if not args.skip_large:
        args.calls, args.device_calls = max(1, args.calls // 5), max(1, args.device_calls // 5)
        built, shapes = catalogue(275696, 128, args.large_users, args.large_users, args, min(args.rounds, 3), 1)      # (a build of the large index takes seconds: one window)
        res["builds"].append(built)
        res["shapes"] += shapes
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
