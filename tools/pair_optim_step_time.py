"""What the optimizer options of the pair trainers cost per training step (A/B tool, not a test; tools/ncf_model_step_time.py's protocol):

    timeout -k 10 600 python tools/pair_optim_step_time.py [--pairs 128] [--rounds 5] [--steps 300] [--out PATH]

scripts/run_ncf.sh's shape: the PMGT_NCF head (64, 2, NeuMF-end) (d = 128), 128 pairs a step, 50 000 users, 7 252 items, the item table
trained with the head (NcfHeadTrainer(train_table=True)), clipping at 5.  Six sides in ONE process over the same pool of uploaded batches,
each on a model of its own with the same initial weights:
  parent           the step as it was before the options existed, restated: the gradient entry + pmgt_op_adamw by hand on a trainer's buffers
  default          NcfHeadTrainer.step with every option at its default (the same entry on the same buffers)
  adamw_sched_grd  AdamW under `linear` with warm-up, nonfinite="skip", step_log=64: pmgt_op_adamw_guarded
  sgd              optim="sgd": pmgt_op_sgd, no schedule, no guard
  sgd_sched_grd    optim="sgd" under `linear` with warm-up, nonfinite="skip", step_log=64
  torch_sgd        the head's formula in torch on the device, autograd (dense embedding gradients), clip_grad_norm_, torch.optim.SGD, LambdaLR
All are warmed up by one window; then they alternate in windows of `steps` steps (the order reversed every other round), each window timed
with device events on the launch stream.  Prints one JSON line: per side the median, minimum, maximum and every window's microseconds per
step, and whether the default side's median lies inside the parent side's own window-to-window range; then pmgt_op_sgd and pmgt_op_adamw
ALONE (op_alone: no gradient entry) at the run's parameter count and at 2^27 floats, with the rate SGD's 17 bytes a parameter come to.  Run
it under a time limit, as above.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pmgt_amd import _lib  # noqa: E402
from pmgt_amd.configuration_pmgt import PMGTConfig  # noqa: E402
from pmgt_amd.ncf_train import TABLE_KEY, NcfHeadTrainer, head_state  # noqa: E402
from pmgt_amd.pmgt_ncf import PMGT_NCF  # noqa: E402
from pmgt_amd.schedule import lr_lambda  # noqa: E402

FACTOR, LAYERS, KIND, USERS, ITEMS = 64, 2, "NeuMF-end", 50000, 7252
D = FACTOR << (LAYERS - 1)
LR, WD, CLIP, POOL = 1e-4, 0.01, 5.0, 16
SCHEDULE = dict(scheduler_type="linear", num_warmup_steps=1000, num_training_steps=1000000)
GUARD = dict(nonfinite="skip", step_log=64)


def window_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def make_model():
    torch.manual_seed(0)
    cfg = PMGTConfig(hidden_size=D, num_hidden_layers=1, num_attention_heads=4, intermediate_size=D, hidden_dropout_prob=0.0,
                     attention_probs_dropout_prob=0.0, beta=0.5)
    return PMGT_NCF(user_num=USERS, item_num=ITEMS, factor_num=FACTOR, num_layers=LAYERS, model=KIND, config=cfg, dtype="fp32")


def make_trainer(table, **options):
    return NcfHeadTrainer(make_model(), table, lr=LR, weight_decay=WD, max_grad_norm=CLIP, train_table=True, **options)


def torch_side(table, pool):
    """step(i) of the head over a trained table in torch on the device: SGD, coupled decay on everything but the biases"""
    p = {k: v.detach().clone().requires_grad_(True) for k, v in head_state(make_model()).items()}
    p[TABLE_KEY] = table.detach().clone().requires_grad_(True)
    opt = torch.optim.SGD([{"params": [v for k, v in p.items() if not k.endswith(".bias")], "weight_decay": WD},
                           {"params": [v for k, v in p.items() if k.endswith(".bias")], "weight_decay": 0.0}], lr=LR)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda(SCHEDULE["scheduler_type"], SCHEDULE["num_warmup_steps"],
                                                             SCHEDULE["num_training_steps"], LR))

    def step(i):
        users, items, labels = pool[i % len(pool)]
        x = torch.cat([p["mlp_user_embeddings.weight"][users], p[TABLE_KEY][items]], dim=-1)
        for layer in range(LAYERS):
            x = torch.relu(x @ p[f"mlp_layers.{layer}.linear.weight"].T + p[f"mlp_layers.{layer}.linear.bias"])
        x = torch.cat([p["gmf_user_embeddings.weight"][users] * p["gmf_item_embeddings.weight"][items], x], dim=-1)
        logits = (x @ p["predict_layer.weight"].T + p["predict_layer.bias"]).view(-1)
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, labels)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(list(p.values()), CLIP)
        opt.step()
        sched.step()
    return step


def op_alone(n, rounds, calls=100):
    """pmgt_op_sgd and pmgt_op_adamw alone on `n` floats (all three launches of each), alternating windows of `calls` calls -> microseconds
    per call, and for SGD the bytes it needs over that time: 4 n read by the norm kernel, 13 n moved by the update."""
    lib = _lib.hip()
    p, g, m, v = (torch.randn(n, device="cuda") * 0.01 for _ in range(4))
    v.abs_()
    dec = (torch.rand(n, device="cuda") < 0.9).to(torch.uint8)
    step, scal, part = torch.zeros(1, dtype=torch.int64, device="cuda"), torch.zeros(8, device="cuda"), torch.zeros(1024, device="cuda")
    tail = (step.data_ptr(), scal.data_ptr(), part.data_ptr())
    sgd = lambda i: _lib.check(lib.pmgt_op_sgd(p.data_ptr(), g.data_ptr(), dec.data_ptr(), n, LR, WD, CLIP, *tail, None, None, _lib.stream()))
    adamw = lambda i: _lib.check(lib.pmgt_op_adamw(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), dec.data_ptr(), n, LR, WD, 0.9, 0.999,
                                                   1e-8, CLIP, *tail, _lib.stream()))
    sides = {"pmgt_op_sgd": (sgd, []), "pmgt_op_adamw": (adamw, [])}
    for name in sides:
        window_us(sides[name][0], calls)
    for r in range(rounds):
        for name in (list(sides) if r % 2 == 0 else list(sides)[::-1]):
            sides[name][1].append(window_us(sides[name][0], calls))
    out = {"n": n}
    for name, (_, us) in sides.items():
        out[name] = {"median": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1)}
    out["sgd_bytes"] = 17 * n
    out["sgd_tb_per_s"] = round(17 * n / (out["pmgt_op_sgd"]["median"] * 1e-6) / 1e12, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pair_optim_step_time.py needs a HIP device")
    rng = np.random.default_rng(0)
    pool = [(torch.from_numpy(rng.integers(0, USERS, size=args.pairs)).cuda(), torch.from_numpy(rng.integers(0, ITEMS, size=args.pairs)).cuda(),
             torch.from_numpy((rng.random(args.pairs) < 0.2).astype(np.float32)).cuda()) for _ in range(POOL)]
    table = torch.from_numpy(rng.standard_normal((ITEMS, D)).astype(np.float32) * 0.1).cuda()
    trainers = {"parent": make_trainer(table), "default": make_trainer(table), "adamw_sched_grd": make_trainer(table, **SCHEDULE, **GUARD),
                "sgd": make_trainer(table, optim="sgd"), "sgd_sched_grd": make_trainer(table, optim="sgd", **SCHEDULE, **GUARD)}
    losses = {name: torch.zeros(1, device="cuda") for name in trainers}
    for t in trainers.values():
        t.grad_fn.reserve(args.pairs)
        t._logits(args.pairs)

    def parent_step(i):                                      # PairTrainer.step as it stood before the options
        t = trainers["parent"]
        users, items, labels = pool[i % len(pool)]
        t.grad_fn(users, items, labels, loss=losses["parent"], logits=t._logits(int(users.shape[0])))
        _lib.check(t.grad_fn.lib.pmgt_op_adamw(t.params.data_ptr(), t.grads.data_ptr(), t.exp_avg.data_ptr(), t.exp_avg_sq.data_ptr(),
                                               t.decay.data_ptr(), t.count, t.lr, t.weight_decay, t.betas[0], t.betas[1], t.eps, t.max_grad_norm,
                                               t.step_count.data_ptr(), t._scal.data_ptr(), t._part.data_ptr(), _lib.stream()))

    def stepper(name):
        return lambda i: trainers[name].step(*pool[i % len(pool)], loss=losses[name])

    sides = {"parent": (parent_step, [])}
    sides.update({name: (stepper(name), []) for name in trainers if name != "parent"})
    sides["torch_sgd"] = (torch_side(table, pool), [])
    order = list(sides)
    for name in order:                                       # warm-up windows, not recorded
        window_us(sides[name][0], args.steps)
    for r in range(args.rounds):
        for name in (order if r % 2 == 0 else order[::-1]):
            sides[name][1].append(window_us(sides[name][0], args.steps))
    torch.cuda.synchronize()
    res = {"metric": "pair_optim_step_time", "head": [FACTOR, LAYERS, KIND], "pairs": args.pairs, "users": USERS, "items": ITEMS,
           "parameters": trainers["default"].count, "steps_per_window": args.steps, "rounds": args.rounds, "pool": POOL, "sides": {}}
    for name, (_, us) in sides.items():
        res["sides"][name] = {"median": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1),
                              "windows": [round(x, 1) for x in us]}
    par, dflt = res["sides"]["parent"], res["sides"]["default"]
    res["default_inside_parent_range"] = bool(par["min"] <= dflt["median"] <= par["max"])
    res["skipped"] = {name: t.step_counters() for name, t in trainers.items() if t.step_counters() is not None}
    res["final_loss"] = {name: float(v[0]) for name, v in losses.items()}
    # the optimizer entries alone: at this run's parameter count (17 bytes a parameter = 188 MB a call: inside the 256 MiB Infinity Cache) and at 2^27 floats (2.28 GB)
    res["op_alone"] = [op_alone(trainers["default"].count, args.rounds), op_alone(1 << 27, args.rounds)]
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
