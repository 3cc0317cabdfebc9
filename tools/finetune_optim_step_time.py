"""What the optimizer options of the fine-tune trainer (PmgtNcfOptionsTrainer) cost per training step, eager and replayed (A/B tool, not a test;
tools/pair_optim_step_time.py's protocol on tools/finetune_step_time.py's shape):

    timeout -k 10 900 python tools/finetune_optim_step_time.py [--pairs 128] [--rounds 5] [--steps 300] [--out PATH]

The README's fine-tune shape: head (64, 2, NeuMF-end), so hidden 128; 4 layers, 8 heads, S = 32; bf16; 128 pairs a step; 50 000 users; the
7 252-node graph of BASELINE.json; lr 1e-4, clip 5, the encoder's dropout on.  Sides in ONE process over the same pool of
uploaded finetune_batches, each on a model of its own with the same initial weights:
  parent                  the step as it was before the options existed, restated: the trainer's gradient pass + pmgt_op_adamw_segments by hand
  default                 PmgtNcfOptionsTrainer.step with every option at its default (the same entry on the same kind of buffers)
  adamw_sched_grd         AdamW under `linear` with warm-up, nonfinite="skip", step_log=64: pmgt_op_step_segments
  sgd                     optim="sgd": pmgt_op_step_segments, no schedule, no guard
  sgd_sched_grd           optim="sgd" under `linear` with warm-up, nonfinite="skip", step_log=64
  <side>_replay           the four trainer sides through capture_step / replay_step: the batch copied into the static buffers (five small
                          copies, as fit_pmgt_ncf(graph=True) feeds a step), then one graph launch
All are warmed up by one window; then they alternate in windows of `steps` steps (the order reversed every other round), each window timed
with device events on the launch stream.  Prints one JSON line: per side the median, minimum, maximum and every window's microseconds per
step, and whether the default side's median lies inside the parent side's own window-to-window range; then the optimizer entries ALONE
(op_alone: no gradient pass) on the default trainer's own segments: pmgt_op_adamw_segments against pmgt_op_step_segments as AdamW without
options, as AdamW scheduled + guarded and as SGD; and the bytes of optimizer state an SGD trainer does not allocate.  Run it under a time
limit, as above.  Needs a GPU; there is no fallback."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pmgt_amd import _lib  # noqa: E402
from pmgt_amd.configuration_pmgt import PMGTConfig  # noqa: E402
from pmgt_amd.datasets import MCNSampler  # noqa: E402
from pmgt_amd.finetune import PmgtNcfOptionsTrainer, finetune_batches  # noqa: E402
from pmgt_amd.graph import synthetic_graph  # noqa: E402
from pmgt_amd.models import synthetic_features  # noqa: E402
from pmgt_amd.pmgt_ncf import PMGT_NCF  # noqa: E402

NODES, EDGES, L, H, S = 7252, 88606, 4, 8, 32              # BASELINE.json configs[1]: the graph; bench.py's c2 depth and context length
FACTOR, HEAD_LAYERS, KIND, USERS = 64, 2, "NeuMF-end", 50000
D = FACTOR << (HEAD_LAYERS - 1)
LR, CLIP, POOL = 1e-4, 5.0, 16
SCHEDULE = dict(scheduler_type="linear", num_warmup_steps=1000, num_training_steps=1000000)
GUARD = dict(nonfinite="skip", step_log=64)
OPTIONS = {"default": {}, "adamw_sched_grd": dict(**SCHEDULE, **GUARD), "sgd": dict(optim="sgd"),
           "sgd_sched_grd": dict(optim="sgd", **SCHEDULE, **GUARD)}


def window_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def make_trainer(feats, pairs, **options):
    torch.manual_seed(0)
    cfg = PMGTConfig(hidden_size=D, num_hidden_layers=L, num_attention_heads=H, intermediate_size=D, hidden_dropout_prob=0.1,
                     attention_probs_dropout_prob=0.1, beta=0.5)
    model = PMGT_NCF(user_num=USERS, item_num=NODES, factor_num=FACTOR, num_layers=HEAD_LAYERS, model=KIND, config=cfg, dtype="bf16")
    model.set_features(feats)
    trainer = PmgtNcfOptionsTrainer(model, lr=LR, max_grad_norm=CLIP, **options)
    trainer.reserve(pairs, S)
    return trainer


def stats(us):
    return {"median": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1), "windows": [round(x, 1) for x in us]}


def op_alone(t, rounds, calls=300):
    """The optimizer entries alone on trainer `t`'s own segments and gradients (whatever its last step left there): alternating windows of
    `calls` calls -> microseconds per call."""
    lib = _lib.hip()
    counters = torch.zeros(4 + 64 * (2 + _lib.STEP_LOG_FLOATS // 2), dtype=torch.int64, device="cuda")
    base = counters.data_ptr()
    guard = _lib.StepGuardC(base, base + 8 * (4 + 2 * 64), base + 32, 64, t._loss.data_ptr(), 1)
    sched = _lib.LrScheduleC(_lib.LR_SCHEDULE_TYPES.index("linear"), 1000, 1000000)
    hyper = (t.lr, t.weight_decay, t.betas[0], t.betas[1], t.eps, t.max_grad_norm)
    tail = (t.step_count.data_ptr(), t._scal.data_ptr(), t._part.data_ptr())
    n = len(t._segs)
    calls_of = {
        "pmgt_op_adamw_segments": lambda i: _lib.check(lib.pmgt_op_adamw_segments(t._segs, n, *hyper, *tail, _lib.stream())),
        "step_segments_adamw": lambda i: _lib.check(lib.pmgt_op_step_segments(t._segs, n, 0, *hyper, *tail, None, None, _lib.stream())),
        "step_segments_adamw_sched_grd": lambda i: _lib.check(lib.pmgt_op_step_segments(t._segs, n, 0, *hyper, *tail, C.byref(sched),
                                                                                        C.byref(guard), _lib.stream())),
        "step_segments_sgd": lambda i: _lib.check(lib.pmgt_op_step_segments(t._segs, n, 1, *hyper, *tail, None, None, _lib.stream())),
    }
    us = {name: [] for name in calls_of}
    for name, fn in calls_of.items():
        window_us(fn, calls)
    for r in range(rounds):
        for name in (list(calls_of) if r % 2 == 0 else list(calls_of)[::-1]):
            us[name].append(window_us(calls_of[name], calls))
    out = {"segments": n, "floats": int(sum(s.n for s in t._segs)), "calls_per_window": calls}
    out.update({name: stats(v) for name, v in us.items()})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("finetune_optim_step_time.py needs a HIP device")
    feats = synthetic_features(NODES, seed=0)
    sampler = MCNSampler(synthetic_graph(NODES, EDGES, seed=0), max_ctx_neigh=S - 1)
    rng = np.random.default_rng(0)
    pairs = np.unique(np.stack([rng.integers(0, USERS, size=POOL * args.pairs), rng.integers(0, NODES, size=POOL * args.pairs)], 1), axis=0)
    pool = []
    for b in finetune_batches(pairs, sampler, USERS, NODES, args.pairs, 1, 0, 0):
        if len(b[0]) == args.pairs and len(pool) < POOL:
            pool.append([torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in b])

    trainers = {"parent": make_trainer(feats, args.pairs)}
    trainers.update({name: make_trainer(feats, args.pairs, **kw) for name, kw in OPTIONS.items()})
    trainers.update({name + "_replay": make_trainer(feats, args.pairs, **kw) for name, kw in OPTIONS.items()})
    losses = {name: torch.zeros(1, device="cuda") for name in trainers}
    statics = {name: t.capture_step(args.pairs, S) for name, t in trainers.items() if name.endswith("_replay")}

    def parent_step(i):                                      # PmgtNcfTrainer.step as it stood before the options
        t = trainers["parent"]
        t._gradients(*pool[i % len(pool)], losses["parent"])
        _lib.check(t.engine.lib.pmgt_op_adamw_segments(t._segs, len(t._segs), t.lr, t.weight_decay, t.betas[0], t.betas[1], t.eps, t.max_grad_norm,
                                                       t.step_count.data_ptr(), t._scal.data_ptr(), t._part.data_ptr(), _lib.stream()))

    def eager(name):
        return lambda i: trainers[name].step(*pool[i % len(pool)], loss=losses[name])

    def replayed(name):
        def step(i):
            for buf, x in zip(statics[name], pool[i % len(pool)]):
                buf.copy_(x)
            trainers[name].replay_step()
        return step

    sides = {"parent": (parent_step, [])}
    sides.update({name: ((replayed if name.endswith("_replay") else eager)(name), []) for name in trainers if name != "parent"})
    order = list(sides)
    for name in order:                                       # warm-up windows, not recorded
        window_us(sides[name][0], args.steps)
    for r in range(args.rounds):
        for name in (order if r % 2 == 0 else order[::-1]):
            sides[name][1].append(window_us(sides[name][0], args.steps))
    torch.cuda.synchronize()
    dflt = trainers["default"]
    moments = 2 * 4 * (dflt.count + sum(hi - lo for lo, hi in dflt.segments))
    res = {"metric": "finetune_optim_step_time", "head": [FACTOR, HEAD_LAYERS, KIND], "hidden": D, "layers": L, "heads": H, "S": S, "dtype": "bf16",
           "pairs": args.pairs, "users": USERS, "nodes": NODES, "steps_per_window": args.steps, "rounds": args.rounds, "pool": len(pool),
           "optimizer_buffers": len(dflt._segs), "head_parameters": dflt.count, "encoder_parameters": sum(hi - lo for lo, hi in dflt.segments),
           "moment_bytes_sgd_does_not_allocate": moments, "sides": {name: stats(us) for name, (_, us) in sides.items()}}
    par, d = res["sides"]["parent"], res["sides"]["default"]
    res["default_inside_parent_range"] = bool(par["min"] <= d["median"] <= par["max"])
    res["skipped"] = {name: t.step_counters() for name, t in trainers.items() if t.step_counters() is not None}
    res["final_loss"] = {name: float(statics[name][5][0]) if name in statics else float(v[0]) for name, v in losses.items()}
    res["op_alone"] = op_alone(dflt, args.rounds)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
