"""What one fine-tuning step of a PMGT_NCF costs on the device, PmgtNcfTrainer.step against the autograd path (A/B tool, not a test):

    python tools/finetune_step_time.py [--pairs 128] [--rounds 5] [--steps 300] [--out PATH]

The reference's shape: head (64, 2, NeuMF-end), so hidden 128; 4 layers, 8 heads, S = 32; bf16; 128 pairs a step; 50 000 users; the
7 252-node graph of BASELINE.json.  Two models with the same initial weights in ONE process, over the same pool of uploaded
finetune_batches:
  trainer    PmgtNcfTrainer.step (lr 1e-4, clip 5): encoder forward, gather, head, scatter, encoder backward, one segmented clip + AdamW
  autograd   PMGT_NCF.forward + binary_cross_entropy_with_logits + backward + clip_grad_norm_ over every trained tensor + AdamW: the
             encoder by pmgt_amd.optimizers.get_optimizer's fused step (all that optimizer can hold is the engine's buffer), the head by
             torch.optim.AdamW
Both are warmed up by one window; then they alternate in windows of `steps` steps, each window timed with device events on the launch
stream.  Prints one JSON line: median, minimum and every window's microseconds per step of both paths, and the launches per step counted
from the code (the trainer's glue, head and optimizer launches are fixed by the entries; the encoder's launch groups are read from the
engine's own recorder over one forward + backward).  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pmgt_amd.configuration_pmgt import PMGTConfig  # noqa: E402
from pmgt_amd.datasets import MCNSampler  # noqa: E402
from pmgt_amd.finetune import PmgtNcfTrainer, finetune_batches  # noqa: E402
from pmgt_amd.graph import synthetic_graph  # noqa: E402
from pmgt_amd.models import synthetic_features  # noqa: E402
from pmgt_amd.optimizers import get_optimizer  # noqa: E402
from pmgt_amd.pmgt_ncf import PMGT_NCF  # noqa: E402

NODES, EDGES, L, H, S = 7252, 88606, 4, 8, 32              # BASELINE.json configs[1]: the graph; bench.py's c2 depth and context length
FACTOR, HEAD_LAYERS, KIND, USERS = 64, 2, "NeuMF-end", 50000
D = FACTOR << (HEAD_LAYERS - 1)
LR, CLIP, POOL = 1e-4, 5.0, 16


def window_us(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / n


def make_model(feats):
    torch.manual_seed(0)
    cfg = PMGTConfig(hidden_size=D, num_hidden_layers=L, num_attention_heads=H, intermediate_size=D, hidden_dropout_prob=0.1,
                     attention_probs_dropout_prob=0.1, beta=0.5)
    model = PMGT_NCF(user_num=USERS, item_num=NODES, factor_num=FACTOR, num_layers=HEAD_LAYERS, model=KIND, config=cfg, dtype="bf16")
    model.set_features(feats)
    return model


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("finetune_step_time.py needs a HIP device")
    feats = synthetic_features(NODES, seed=0)
    sampler = MCNSampler(synthetic_graph(NODES, EDGES, seed=0), max_ctx_neigh=S - 1)
    rng = np.random.default_rng(0)
    pairs = np.unique(np.stack([rng.integers(0, USERS, size=POOL * args.pairs), rng.integers(0, NODES, size=POOL * args.pairs)], 1), axis=0)
    pool = []
    for b in finetune_batches(pairs, sampler, USERS, NODES, args.pairs, 1, 0, 0):
        if len(b[0]) == args.pairs and len(pool) < POOL:
            pool.append([torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in b])

    model_t, model_a = make_model(feats), make_model(feats)
    trainer = PmgtNcfTrainer(model_t, lr=LR, max_grad_norm=CLIP)
    trainer.reserve(args.pairs, S)
    loss_t = torch.zeros(1, device="cuda")

    def step_trainer(i):
        trainer.step(*pool[i % len(pool)], loss=loss_t)

    model_a.train()
    trained = [p for p in model_a.parameters() if p.requires_grad]
    head = [p for k, p in model_a.named_parameters() if p.requires_grad and not k.startswith("bert.")]
    enc_opt = get_optimizer(types.SimpleNamespace(model=model_a.bert, decay=0.0, lr=LR, optim="adamw", gradient_max_norm=None))
    head_opt = torch.optim.AdamW(head, lr=LR, weight_decay=0.0)

    def step_autograd(i):
        users, items, labels, node_ids, mask = pool[i % len(pool)]
        logits = model_a(users, {"node_ids": node_ids, "attention_mask": mask})
        loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, labels)
        enc_opt.zero_grad(), head_opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(trained, CLIP)
        enc_opt.step(), head_opt.step()

    sides = {"trainer": (step_trainer, []), "autograd": (step_autograd, [])}
    for name in sides:                                        # warm-up windows, not recorded
        window_us(sides[name][0], args.steps)
    for r in range(args.rounds):
        for name in (("trainer", "autograd") if r % 2 == 0 else ("autograd", "trainer")):
            sides[name][1].append(window_us(sides[name][0], args.steps))
    torch.cuda.synchronize()

    groups = None
    try:                                                      # the encoder's launch groups of one forward + backward, from the engine's recorder
        model_t.engine.profile_begin()
        trainer.grad(*pool[0])
        groups = len(model_t.engine.profile_sequence())
        model_t.engine.profile_end()
    except RuntimeError as e:
        groups = f"not counted ({e})"
    k = len(trainer.segments) + 1
    res = {"metric": "finetune_step_time", "head": [FACTOR, HEAD_LAYERS, KIND], "hidden": D, "layers": L, "heads": H, "S": S, "dtype": "bf16",
           "pairs": args.pairs, "users": USERS, "nodes": NODES, "steps_per_window": args.steps, "pool": len(pool),
           "launches_per_step": {"cls_gather": 1, "head": 2, "cls_scatter": 1, "optimizer": 2 * k + 1, "optimizer_buffers": k,
                                 "encoder_launch_groups": groups}}
    for name, (_, us) in sides.items():
        res[f"{name}_us"] = {"median": round(statistics.median(us), 1), "min": round(min(us), 1), "max": round(max(us), 1),
                             "windows": [round(x, 1) for x in us]}
    res["autograd_over_trainer"] = round(res["autograd_us"]["median"] / res["trainer_us"]["median"], 3)
    res["final_loss_trainer"] = float(loss_t[0])
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
