"""What the per-step exponential weight average costs a captured C2 step (A/B tool, not a test):

    python tools/weight_average_cost.py [--batch 1024] [--rounds 6] [--replays 40] [--out PATH]

bench.py's flagship configuration (workload c2, bf16, dropout 0.1, B = 1024, lr 1e-4, clip 5) on two engines in ONE process: a trainer
without averaging and one with weight_average=dict(mode="ema").  Each captures its step over the same staged batch; the two graphs are
then replayed in alternating windows of `replays` steps, each window timed with device events on the launch stream (warm-up windows
first), so both see the same box at the same time.  Prints one JSON line: the median, minimum and every window's ms per step of both, the
difference of the medians, and the same A/B for the update alone (the two launches of WeightAverage.update, eager, event-timed) with its
byte count (12 bytes per parameter: read p, read avg, write avg).  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pmgt_amd.configuration_pmgt import PMGTConfig  # noqa: E402
from pmgt_amd.datasets import MODE_TRAIN, MCNSampler  # noqa: E402
from pmgt_amd.engine import Engine  # noqa: E402
from pmgt_amd.graph import synthetic_graph  # noqa: E402
from pmgt_amd.models import reference_init, synthetic_features  # noqa: E402
from pmgt_amd.trainer import Trainer  # noqa: E402

NODES, EDGES, L, H, D, I, S = 7252, 88606, 4, 8, 256, 256, 32      # bench.py WORKLOADS["c2"]


def window_ms(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--replays", type=int, default=40)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("weight_average_cost.py needs a HIP device")
    cfg = PMGTConfig(hidden_size=D, num_hidden_layers=L, num_attention_heads=H, intermediate_size=I, hidden_dropout_prob=0.1,
                     attention_probs_dropout_prob=0.1, beta=0.5)
    graph = synthetic_graph(NODES, EDGES, seed=0)
    vis, txt = synthetic_features(NODES, seed=0)
    smp = MCNSampler(graph, max_ctx_neigh=S - 1)
    tgt, pair, num_pairs, labels = smp.batch(np.arange(2, 2 + args.batch), MODE_TRAIN, threads=8, base_seed=0, counter=0)
    cu = lambda d: {k: v.cuda() for k, v in d.items()}
    batch = (cu(tgt), cu(pair), num_pairs.cuda(), labels.cuda())
    sides = {}
    for name, wa in (("off", None), ("on", dict(mode="ema", decay=0.999, warmup=True))):
        eng = Engine(cfg, dtype="bf16", device="cuda:0", seed=1234)
        reference_init(eng, seed=0)
        eng.set_tables(vis, txt)
        tr = Trainer(eng, lr=1e-4, weight_decay=1e-2, max_grad_norm=5.0, weight_average=wa)
        sides[name] = dict(eng=eng, tr=tr, replay=tr.capture_step(batch, warmup=3), ms=[])
    for name in ("off", "on"):                                  # warm-up windows, not recorded
        window_ms(sides[name]["replay"], args.replays)
    for r in range(args.rounds):
        for name in (("off", "on") if r % 2 == 0 else ("on", "off")):
            sides[name]["ms"].append(window_ms(sides[name]["replay"], args.replays))
    torch.cuda.synchronize()
    wa = sides["on"]["tr"].weight_average
    window_ms(wa.update, 50)
    upd = [window_ms(wa.update, 200) for _ in range(5)]
    n = sides["on"]["eng"].n_params
    res = {"metric": "weight_average_cost", "workload": "c2", "batch": args.batch, "n_params": int(n), "replays_per_window": args.replays}
    for name in ("off", "on"):
        ms = sides[name]["ms"]
        res[f"step_ms_{name}"] = {"median": round(statistics.median(ms), 4), "min": round(min(ms), 4), "windows": [round(x, 4) for x in ms]}
    res["delta_ms_of_medians"] = round(res["step_ms_on"]["median"] - res["step_ms_off"]["median"], 4)
    res["delta_percent"] = round(100.0 * res["delta_ms_of_medians"] / res["step_ms_off"]["median"], 3)
    res["update_alone_us"] = {"median": round(statistics.median(upd) * 1e3, 2), "min": round(min(upd) * 1e3, 2), "bytes": int(12 * n),
                              "launches": 2}
    res["ema_updates_counted"] = wa.count()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    del sides
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
