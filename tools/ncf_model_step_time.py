"""What one training step of the stand-alone NCF model costs on the device, NcfModelTrainer.step against the autograd path (A/B tool, not a
test; tools/finetune_step_time.py's protocol):

    python tools/ncf_model_step_time.py [--pairs 128] [--rounds 5] [--steps 300] [--out PATH]

The reference's shape: factor_num 64, 2 layers (d = 128), 128 pairs a step, 50 000 users, 7 252 items, the items trained, clipping at 5.
Four cases: kind NeuMF-end with LayerNorm and kind GMF, each without dropout and with p = 0.2 everywhere (emb_dropout and dropout).  Per
case two models with the same initial weights in ONE process over the same pool of uploaded batches:
  trainer    NcfModelTrainer.step (lr 1e-4, clip 5): pmgt_ncf_model_train_grad (two launches) + pmgt_op_adamw (three)
  autograd   pmgt_amd.ncf.NCF.forward + binary_cross_entropy_with_logits + backward + clip_grad_norm_ + torch.optim.AdamW (dense
             embedding gradients, as the reference trains), in train() mode when the case has dropout
Both are warmed up by one window; then they alternate in windows of `steps` steps, each window timed with device events on the launch
stream.  Prints one JSON line: per case the median, minimum, maximum and every window's microseconds per step of both paths.  Needs a GPU;
there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pmgt_amd.ncf import NCF  # noqa: E402
from pmgt_amd.ncf_model_train import NcfModelTrainer  # noqa: E402

FACTOR, LAYERS, USERS, ITEMS = 64, 2, 50000, 7252
LR, CLIP, POOL = 1e-4, 5.0, 16
CASES = [("neumf_ln", "NeuMF-end", True, 0.0), ("neumf_ln_p02", "NeuMF-end", True, 0.2), ("gmf", "GMF", False, 0.0), ("gmf_p02", "GMF", False, 0.2)]


def window_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def make_model(kind, ln, p):
    torch.manual_seed(0)
    return NCF(USERS, ITEMS, FACTOR, LAYERS, emb_dropout=p, dropout=p, use_layer_norm=ln, model=kind).cuda()


def measure(kind, ln, p, pool, rounds, steps):
    model_t, model_a = make_model(kind, ln, p), make_model(kind, ln, p)
    trainer = NcfModelTrainer(model_t, lr=LR, max_grad_norm=CLIP, dropout_seed=1 if p else None)
    trainer.grad_fn.reserve(len(pool[0][0]))
    loss_t = torch.zeros(1, device="cuda")

    def step_trainer(i):
        trainer.step(*pool[i % len(pool)], loss=loss_t)

    model_a.train(bool(p))
    opt = torch.optim.AdamW([q for q in model_a.parameters()], lr=LR, weight_decay=0.0)

    def step_autograd(i):
        users, items, labels = pool[i % len(pool)]
        loss = torch.nn.functional.binary_cross_entropy_with_logits(model_a((users, items)), labels)
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_([q for q in model_a.parameters() if q.grad is not None], CLIP)
        opt.step()

    sides = {"trainer": (step_trainer, []), "autograd": (step_autograd, [])}
    for name in sides:                                        # warm-up windows, not recorded
        window_us(sides[name][0], steps)
    for r in range(rounds):
        for name in (("trainer", "autograd") if r % 2 == 0 else ("autograd", "trainer")):
            sides[name][1].append(window_us(sides[name][0], steps))
    torch.cuda.synchronize()
    res = {"kind": kind, "layer_norm": ln, "p": p, "parameters": trainer.count, "launches_per_step": {"gradient": 2, "optimizer": 3}}
    for name, (_, us) in sides.items():
        res[f"{name}_us"] = {"median": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1),
                             "windows": [round(x, 1) for x in us]}
    res["autograd_over_trainer"] = round(res["autograd_us"]["median"] / res["trainer_us"]["median"], 3)
    res["final_loss_trainer"] = float(loss_t[0])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("ncf_model_step_time.py needs a HIP device")
    rng = np.random.default_rng(0)
    pool = [(torch.from_numpy(rng.integers(0, USERS, size=args.pairs)).cuda(), torch.from_numpy(rng.integers(0, ITEMS, size=args.pairs)).cuda(),
             torch.from_numpy((rng.random(args.pairs) < 0.2).astype(np.float32)).cuda()) for _ in range(POOL)]
    res = {"metric": "ncf_model_step_time", "factor_num": FACTOR, "num_layers": LAYERS, "pairs": args.pairs, "users": USERS, "items": ITEMS,
           "steps_per_window": args.steps, "pool": POOL, "cases": {}}
    for tag, kind, ln, p in CASES:
        res["cases"][tag] = measure(kind, ln, p, pool, args.rounds, args.steps)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
