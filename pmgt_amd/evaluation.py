"""Evaluation and export over the engine's forward pass: the validation pass with its ROC AUC on the host or on the device, and the
embedding export (reference: `_validation_and_test_step`, `_valid_and_test_epoch_end` and `inference`, pmgt/pmgt/trainer.py:153-195,259-275);
the top-N ranking evaluation of the downstream model, nDCG@k / Recall@k per user on the host or on the device (reference:
`NCFTrainerModel._validation_and_test_step` and `validation_epoch_end`, pmgt/ncf/trainer.py:202-254; get_ndcg / get_recall,
pmgt/metrics.py:16-37)."""
import numpy as np
import torch

from .datasets import MODE_EVAL, MODE_INFERENCE
from .ncf_head import check_ids, check_item_table
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


# ---- top-N ranking: nDCG@k / Recall@k per user ------------------------------------------------------------------------------------------------
def score_key(scores: np.ndarray) -> np.ndarray:
    """eval_key() of pmgt_amd/ops/eval_metrics.h in numpy: -0.0 folded onto +0.0, negative values bit-flipped, the others with the sign
    bit set, so the unsigned order of the keys is the numeric order of the scores (+-inf at the ends).  NaN gets 0xFFFFFFFF."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    b = s.view(np.uint32).copy()
    b[s == 0] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    k = np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)
    k[np.isnan(s)] = np.uint32(0xFFFFFFFF)
    return k


def ranking_metrics_host(logits, labels, counts=None, ks=(10, 20)) -> dict:
    """The "host" path of the ranking metrics and the yardstick of the device path (pmgt_amd.metrics.RankingMetrics), pure numpy, the same
    definitions: per user row, candidates in stable descending order of their key -- among equal scores THE LOWER CANDIDATE INDEX RANKS
    FIRST (torch.topk leaves ties unspecified; this is the project's rule) --, recall_k = hits_k / n_pos, dcg_k = the discounts of the hit
    ranks below k added in ascending rank in fp64, ndcg_k = dcg_k / idcg[min(n_pos, k) - 1], loss = mean over the live candidates of
    max(x, 0) - x y + log1p(exp(-|x|)) in fp32.  logits, labels [U, C]; counts [U] live candidates per row (None = full rows; entries past
    the count are never read into a result).
    -> dict: ndcg[k], recall[k] fp64 [U]; loss fp32 [U]; n_pos int32 [U]; nan, empty bool [U]; order int64 [U, C], the candidates by
    rank (-1 past the count)."""
    from .metrics import check_ks, discount_tables
    ks = check_ks(ks)
    x = np.ascontiguousarray(logits, dtype=np.float32)
    y = np.asarray(labels)
    if x.ndim != 2 or y.shape != x.shape:
        raise ValueError(f"ranking_metrics_host: logits {x.shape} and labels {y.shape} must be one [U, C] shape")
    U, Cn = x.shape
    counts = np.full(U, Cn, dtype=np.int64) if counts is None else np.asarray(counts).astype(np.int64)
    if counts.shape != (U,) or (counts < 0).any() or (counts > Cn).any():
        raise ValueError(f"ranking_metrics_host: counts must be [U] integers in [0, {Cn}]")
    live = np.arange(Cn)[None, :] < counts[:, None]
    pos = (y != 0) & live
    # descending by key, stable: ascending in (2^32 - 1 - key); padding behind every live candidate
    inv = np.where(live, np.int64(0xFFFFFFFF) - score_key(x).astype(np.int64), np.int64(1) << 32)
    order = np.argsort(inv, axis=1, kind="stable")
    rank = np.empty_like(order)
    np.put_along_axis(rank, order, np.broadcast_to(np.arange(Cn), (U, Cn)), axis=1)
    max_k = ks[-1]
    disc, idcg = discount_tables(max_k)
    hit = np.zeros((U, max(max_k, Cn)), dtype=bool)
    rows, cols = np.nonzero(pos)
    hit[rows, rank[rows, cols]] = True
    hit = hit[:, :max_k]
    dcg = np.cumsum(np.where(hit, disc[None, :], 0.0), axis=1)       # sequential along the rank: the adds in ascending order
    nhit = np.cumsum(hit, axis=1)
    n_pos = pos.sum(axis=1).astype(np.int32)
    empty = n_pos == 0
    safe = np.maximum(n_pos, 1)
    out = dict(ndcg={}, recall={})
    for k in ks:
        out["recall"][k] = np.where(empty, 0.0, nhit[:, k - 1].astype(np.float64) / safe)
        out["ndcg"][k] = np.where(empty, 0.0, dcg[:, k - 1] / idcg[np.minimum(safe, k) - 1])
    with np.errstate(over="ignore", invalid="ignore"):
        yb = (y != 0).astype(np.float32)
        term = (np.maximum(x, np.float32(0)) - x * yb) + np.log1p(np.exp(-np.abs(x)))
        term = np.where(live, term, np.float32(0)).astype(np.float32)
        loss = np.where(counts > 0, term.sum(axis=1, dtype=np.float32) / np.maximum(counts, 1).astype(np.float32), np.float32(0))
    out.update(loss=loss.astype(np.float32), n_pos=n_pos, nan=(np.isnan(x) & live).any(axis=1), empty=empty,
               order=np.where(live, order, -1))
    return out


def summarize_ranking(per_user: dict, ks) -> dict:
    """{"n<k>", "r<k>", "loss"}: the means over the users of a per-user dict; raises as RankingMetrics.result() does."""
    n = len(per_user["n_pos"])
    n_nan, n_empty = int(np.count_nonzero(per_user["nan"])), int(np.count_nonzero(per_user["empty"]))
    if n_nan:
        raise ValueError(f"ranking metrics: {n_nan} of {n} users have a NaN logit among their candidates")
    if n_empty:
        raise ValueError(f"ranking metrics: {n_empty} of {n} users have no positive candidate")
    out = {f"n{k}": float(np.mean(per_user["ndcg"][k])) for k in ks}
    out.update({f"r{k}": float(np.mean(per_user["recall"][k])) for k in ks})
    out["loss"] = float(np.mean(per_user["loss"].astype(np.float64)))
    return out


@torch.no_grad()
def encode_catalogue(model, sampler, batch_size: int = 1024, threads: int = 8, seed: int = 0) -> torch.Tensor:
    """The CLS state of every item of `model`'s catalogue through the engine's inference entry, as a DEVICE fp32 table [item_num, d]: the
    contexts and counter-seeded streams of export_embeddings (item j = node j + 2 draws from stream j), nothing copied back."""
    eng = model.engine
    n_items = model.item_num
    table = torch.empty(n_items, eng.config.hidden_size, dtype=torch.float32, device=eng.device)
    ids = np.arange(2, n_items + 2)
    for lo in range(0, n_items, batch_size):
        tg = ids[lo: lo + batch_size]
        tgt = sampler.batch(tg, MODE_INFERENCE, threads=threads, base_seed=seed, counter=lo)
        last, _, _ = eng.encode(ids=tgt["node_ids"].to(eng.device), attention_mask=tgt["attention_mask"].to(eng.device))
        table[lo: lo + len(tg)] = last[:, 0].float()
    return table


@torch.no_grad()
def rank_users(model, table: torch.Tensor, users: torch.Tensor, candidates: torch.Tensor, labels: torch.Tensor, counts: torch.Tensor,
               sink, batch_users: int = 256) -> None:
    """The loop of evaluate_ranking over DEVICE tensors: per batch of users, gather the candidates' rows of `table`, run the torch head of
    PMGT_NCF on [batch * C] pairs and hand the [batch, C] logits to `sink(logits, labels, counts, offset)`.  With RankingMetrics.update as
    the sink nothing in here copies to the host or waits for the device."""
    U, Cn = candidates.shape
    for lo in range(0, U, batch_users):
        hi = min(lo + batch_users, U)
        cand = candidates[lo:hi].reshape(-1)
        user = users[lo:hi, None].expand(hi - lo, Cn).reshape(-1)
        logits = model.head(user, cand, table.index_select(0, cand)).view(hi - lo, Cn)
        sink(logits.contiguous(), labels[lo:hi], counts[lo:hi], lo)


def check_candidates(model, users, candidates, labels, counts, who: str):
    """The four arrays as rank_users reads them; ValueError in `who`'s name for shapes that differ, counts or C out of range, and ids outside
    `model`'s tables (which would only show up as a device-side fault in the gather)."""
    users, candidates = np.ascontiguousarray(users, dtype=np.int64), np.ascontiguousarray(candidates, dtype=np.int64)
    labels, counts = np.ascontiguousarray(labels, dtype=np.float32), np.ascontiguousarray(counts, dtype=np.int32)
    if candidates.ndim != 2 or users.shape != candidates.shape[:1] or labels.shape != candidates.shape or counts.shape != users.shape or len(users) < 1:
        raise ValueError(f"{who}: users {users.shape}, candidates {candidates.shape}, labels {labels.shape}, counts {counts.shape} must be [U], [U, C] x 2, [U]")
    check_ids("users", users, model.user_num, who)
    check_ids("candidates", candidates, model.item_num, who)
    if counts.min() < 1 or counts.max() > candidates.shape[1] or candidates.shape[1] > 4096:
        raise ValueError(f"{who}: counts must lie in [1, C = {candidates.shape[1]}] and C in [1, 4096]")
    return users, candidates, labels, counts


def evaluate_ranking(model, sampler, users, candidates, labels, counts, ks=(10, 20), batch_users: int = 256, metrics: str = "host",
                     threads: int = 8, seed: int = 0, per_user: bool = False, table=None):
    """Top-N recommendation quality of a PMGT_NCF (the reference's test_step / test_epoch_end, pmgt/ncf/trainer.py:202-254): the catalogue
    is encoded ONCE in eval mode (encode_catalogue), every user's candidates (pmgt_amd.datasets.ranking_candidates) are scored by the
    model's head on rows gathered from that table, and the scores are ranked per user -> {"n<k>", "r<k>" for k in ks, "loss"}: mean nDCG@k,
    Recall@k and per-user BCE-with-logits loss.  Ties rank the lower candidate index first.
    metrics="host" (default): the logits of every batch are copied out and ranking_metrics_host ranks them.
    metrics="device": they stay on the device (pmgt_amd.metrics.RankingMetrics, HIP); the loop copies nothing back and never waits, one
    small copy at the end fetches the sums.  Per-user nDCG, recall and n_pos are equal on both paths; the per-user loss may differ in its
    last bits (fp32 summation order) and the means by U * 2^-52 (summation order).
    per_user=True: returns (result, per-user dict) -- ndcg[k], recall[k], loss, n_pos as numpy arrays.
    table: a ready item table (fp32 [item_num, d] on the model's device: encode_catalogue's, or one trained with the head by
    fit_ncf(train_table=True)) to score against instead of encoding the catalogue, as for recommend; `sampler` is then not used."""
    from .metrics import RankingMetrics, check_ks
    if metrics not in ("host", "device"):
        raise ValueError(f"metrics={metrics!r}: expected 'host' or 'device'")
    ks = check_ks(ks)
    users, candidates, labels, counts = check_candidates(model, users, candidates, labels, counts, "evaluate_ranking")
    from .ncf import NCF
    if isinstance(model, NCF):                               # the stand-alone model: its own item table, no encoder (`sampler` is not used)
        dev, width = model.predict_layer.weight.device, model.factor_num << (model.num_layers - 1)
        table = model.embed_item_MLP.weight.detach() if table is None else table
    else:
        dev, width = model.engine.device, model.config.hidden_size
    if table is not None:
        check_item_table(table, model.item_num, width, dev, "evaluate_ranking")
    was_training = model.training
    model.eval()
    try:
        if table is None:
            table = encode_catalogue(model, sampler, threads=threads, seed=seed)
        on_dev = [torch.from_numpy(a).to(dev) for a in (users, candidates, labels, counts)]
        if metrics == "device":
            rm = RankingMetrics(dev, len(users), ks)
            rank_users(model, table, *on_dev, sink=rm.update, batch_users=batch_users)
            result = rm.result()
            return (result, rm.per_user()) if per_user else result
        rows = []
        rank_users(model, table, *on_dev, sink=lambda lg, lb, ct, lo: rows.append(lg.cpu().numpy()), batch_users=batch_users)
    finally:
        model.train(was_training)
    pu = ranking_metrics_host(np.concatenate(rows), labels, counts, ks)
    result = summarize_ranking(pu, ks)
    return (result, pu) if per_user else result
