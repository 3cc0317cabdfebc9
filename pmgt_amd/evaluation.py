"""Evaluation and export over the engine's forward pass: the validation pass with its ROC AUC on the host or on the device, and the
embedding export (reference: `_validation_and_test_step`, `_valid_and_test_epoch_end` and `inference`, pmgt/pmgt/trainer.py:153-195,259-275)."""
import numpy as np
import torch

from .datasets import MODE_EVAL, MODE_INFERENCE
from .parallel import gather_predictions, world


def batch_to_device(batch, device, non_blocking: bool = False):
    """A host batch of MCNSampler.batch (target dict, pair dict, num_pairs, labels) as the same 4-tuple of tensors on `device`."""
    tgt, pair, num_pairs, labels = batch
    to = lambda t: t.to(device, non_blocking=non_blocking)
    return {k: to(v) for k, v in tgt.items()}, {k: to(v) for k, v in pair.items()}, to(num_pairs), to(labels)


def roc_auc_score(labels: np.ndarray, scores: np.ndarray) -> float:
    """sklearn.metrics.roc_auc_score for binary labels (what `_valid_and_test_epoch_end` logs as val/auc,
    pmgt/pmgt/trainer.py:182-195): Mann-Whitney U with midranks for ties."""
    labels = np.asarray(labels).astype(bool)
    scores = np.asarray(scores, dtype=np.float64)
    n_pos, n_neg = int(labels.sum()), int((~labels).sum())
    if n_pos == 0 or n_neg == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    order = np.argsort(scores, kind="mergesort")
    s = scores[order]
    ranks = np.empty(len(s), dtype=np.float64)
    i = 0
    while i < len(s):
        j = i
        while j + 1 < len(s) and s[j + 1] == s[i]:
            j += 1
        ranks[i:j + 1] = 0.5 * (i + j) + 1.0
        i = j + 1
    r = np.empty_like(ranks)
    r[order] = ranks
    return float((r[labels].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


EVAL_PINNED_SLOTS = 4      # evaluate(metrics="device"): pinned batch buffers in flight


def _gather_validation(preds, labs, loss_sum, n_total: int, ws: int):
    """The tail of a validation over ws > 1 ranks: everyone's predictions and labels (ONE transfer per validation), loss sum and count summed."""
    import torch.distributed as dist
    preds, labs = gather_predictions(preds, labs)
    parts = [None] * ws
    dist.all_gather_object(parts, (loss_sum, n_total))
    return preds, labs, sum(p[0] for p in parts), sum(p[1] for p in parts)


def _evaluate_device(engine, sampler, mine: np.ndarray, batch_size: int, threads: int, seed: int, rank: int, ws: int):
    """evaluate(metrics="device"): the same batches through pinned host buffers and non-blocking copies, scores / labels / loss kept on the
    device by a ValidationMetrics.  Nothing in the loop waits for the GPU's compute, so the sampler call of batch k + 1 runs while the GPU
    works on batch k.  The pinned buffers form a ring of EVAL_PINNED_SLOTS: before the sampler overwrites a slot, the host waits for the
    event behind THAT slot's own copies, EVAL_PINNED_SLOTS batches back -- back-pressure that bounds the run-ahead, not a per-batch sync."""
    from .metrics import ValidationMetrics
    dev = engine.device
    vm = ValidationMetrics(dev, max(len(mine) * max(sampler.max_pairs(MODE_EVAL), 1), 1))
    rows = max(min(int(batch_size), len(mine)), 1)
    ring = [dict(buf=sampler.alloc(rows, MODE_EVAL, pinned=True), copied=None) for _ in range(EVAL_PINNED_SLOTS)]
    for k, lo in enumerate(range(0, len(mine), batch_size)):
        tg = mine[lo: lo + batch_size]
        slot = ring[k % EVAL_PINNED_SLOTS]
        if slot["copied"] is not None:
            slot["copied"].synchronize()
        batch = batch_to_device(sampler.batch(tg, MODE_EVAL, out=slot["buf"], threads=threads, base_seed=seed, counter=rank + ws * lo,
                                              counter_stride=ws), dev, non_blocking=True)
        slot["copied"] = torch.cuda.Event()
        slot["copied"].record()
        out = engine.pretrain_step(batch, training=False, want_hidden=False)
        vm.update(out["logits"], batch[3], out["loss"], len(tg))
    if ws > 1:
        preds, labs, loss_sum, n_total = _gather_validation(vm.scores(), vm.labels(), vm.loss_sum(), len(mine), ws)
        vm = ValidationMetrics(dev, max(len(preds), 1))
        if len(preds):
            vm.update_scores(torch.from_numpy(preds).to(dev), torch.from_numpy(labs).to(dev))
        return {"loss/val": float(loss_sum / max(n_total, 1)), "val/auc": vm.result()["val/auc"]}
    return vm.result()


@torch.no_grad()
def evaluate(engine, sampler, node_ids: np.ndarray, batch_size: int = 256, threads: int = 8, seed: int = 0,
             distributed: bool = False, metrics: str = "host"):
    """Validation pass (pmgt/pmgt/trainer.py:162-195): eval-mode forward with 1 positive + 1 negative
    per target, sigmoid(logits) vs labels -> {'loss/val', 'val/auc'}.  `loss/val` is the mean of the per-batch losses
    (what `self.log("loss/val", ...)` aggregates over an epoch, weighted by batch size).  distributed=True under an
    initialised process group: rank r evaluates node_ids[r::W] and the predictions of all ranks are gathered, so every
    rank reports the same AUC over the whole validation set (the reference's AUC is per rank: no sync_dist); every node
    draws from the stream of its GLOBAL index, so the result equals the single-process evaluation of the same list.
    metrics="host" (default): predictions and the loss are copied to the host after every batch and roc_auc_score runs there.
    metrics="device": they stay on the device (pmgt_amd.metrics.ValidationMetrics: sigmoid, loss accumulation, sort and the Mann-Whitney
    statistic in HIP) and one small copy at the end fetches the result; `loss/val` is bit-identical to the host path, `val/auc` is
    roc_auc_score of the scores the device computed, exactly (its sigmoid may differ from torch's in the last bit)."""
    if metrics not in ("host", "device"):
        raise ValueError(f"metrics={metrics!r}: expected 'host' or 'device'")
    node_ids = np.asarray(node_ids)
    rank, ws = world() if distributed else (0, 1)
    mine = node_ids[rank::ws]
    if metrics == "device":
        return _evaluate_device(engine, sampler, mine, batch_size, threads, seed, rank, ws)
    preds, labs = [np.empty(0, np.float32)], [np.empty(0, np.float32)]
    loss_sum = 0.0
    for lo in range(0, len(mine), batch_size):
        tg = mine[lo: lo + batch_size]
        batch = sampler.batch(tg, MODE_EVAL, threads=threads, base_seed=seed, counter=rank + ws * lo,
                              counter_stride=ws)      # item j of this rank = item rank + ws * j of the list
        out = engine.pretrain_step(batch_to_device(batch, engine.device), training=False, want_hidden=False)
        preds.append(torch.sigmoid(out["logits"]).cpu().numpy())
        labs.append(batch[3].numpy())
        loss_sum += out["loss"].item() * len(tg)
    preds, labs = np.concatenate(preds), np.concatenate(labs)
    n_total = len(mine)
    if ws > 1:
        preds, labs, loss_sum, n_total = _gather_validation(preds, labs, loss_sum, n_total, ws)
    return {"loss/val": float(loss_sum / max(n_total, 1)), "val/auc": roc_auc_score(labs, preds)}


@torch.no_grad()
def export_embeddings(engine, sampler, n_nodes: int, batch_size: int = 1024, threads: int = 8, seed: int = 0) -> np.ndarray:
    """Inference / export (pmgt/pmgt/trainer.py:153-154,259-275; pmgt/base_trainer.py:400-407): CLS hidden
    state of every node in id order as fp32 [N, d] (contexts are still randomly sampled, as in the reference)."""
    out = np.empty((n_nodes, engine.config.hidden_size), dtype=np.float32)
    ids = np.arange(2, n_nodes + 2)
    for lo in range(0, n_nodes, batch_size):
        tg = ids[lo: lo + batch_size]
        tgt = sampler.batch(tg, MODE_INFERENCE, threads=threads, base_seed=seed, counter=lo)
        last, _, _ = engine.encode(ids=tgt["node_ids"].to(engine.device), attention_mask=tgt["attention_mask"].to(engine.device))
        out[lo: lo + len(tg)] = last[:, 0].float().cpu().numpy()
    return out
