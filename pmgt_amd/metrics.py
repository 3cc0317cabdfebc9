"""Validation metrics kept on the device (pmgt_eval_* of include/pmgt_capi.h, kernels in ops/eval_metrics.hip): what
`_validation_and_test_step` / `_valid_and_test_epoch_end` collect and compute on the host (pmgt/pmgt/trainer.py:162-195) -- sigmoid(logits)
and labels per batch, the batch loss weighted by its size, roc_auc_score at the end -- with ONE device-to-host copy per validation.

`update` enqueues a kernel and returns; only `result`, `scores`, `labels` and `loss_sum` read from the device.

`RankingMetrics` is the same one level up (pmgt_rank_*, kernels in ops/ranking_metrics.hip): nDCG@k / Recall@k per user over a row of
candidates, what the reference's ranking evaluation computes per user on the host (pmgt/ncf/trainer.py:202-254, pmgt/metrics.py:16-37)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

HEADER_BYTES = 64             # PMGT_EVAL_HEADER_BYTES
MAX_CAPACITY = 1 << 26
ONE_CLASS = "Only one class present in y_true. ROC AUC score is not defined in that case."       # roc_auc_score's text



class ValidationMetrics:
    """`capacity` prediction slots on `device`.  reset() -> update(...) per batch -> result().  The cursor (next free slot) and the number of
    targets are host integers: the host sampler knows every batch's pair count, so nothing is read back to advance them.
    workspace: optional uint8 device tensor of at least `workspace_bytes(capacity)` bytes to use instead of an allocation of its own."""

    def __init__(self, device, capacity: int, workspace: torch.Tensor = None):
        self.lib = _lib.hip()
        self.device = torch.device(device)
        self.capacity = int(capacity)
        if not 1 <= self.capacity <= MAX_CAPACITY:
            raise ValueError(f"ValidationMetrics: capacity = {capacity!r} outside [1, {MAX_CAPACITY}]")
        self.nbytes = self.workspace_bytes(self.capacity)
        if workspace is None:
            workspace = torch.empty(self.nbytes, dtype=torch.uint8, device=self.device)
        if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < self.nbytes:
            raise ValueError(f"ValidationMetrics: the workspace must be a contiguous uint8 tensor of >= {self.nbytes} bytes")
        self._ws = workspace
        self._capr = (self.capacity + 255) // 256 * 256
        self.cursor = 0
        self.n_targets = 0
        self.reset()

    @staticmethod
    def workspace_bytes(capacity: int) -> int:
        n = int(_lib.hip().pmgt_eval_workspace_bytes(int(capacity)))
        if n < 0:
            raise ValueError(f"ValidationMetrics: capacity = {capacity!r} outside [1, {MAX_CAPACITY}]")
        return n

    def reset(self) -> None:
        _lib.check(self.lib.pmgt_eval_reset(self._ws.data_ptr(), self.capacity, _lib.stream()))
        self.cursor = 0
        self.n_targets = 0

    def _append(self, fn, values, labels, loss, n_targets, offset):
        n = int(values.numel())
        off = self.cursor if offset is None else int(offset)
        if off < 0 or off + n > self.capacity:
            raise ValueError(f"ValidationMetrics: predictions [{off}, {off + n}) do not fit the capacity of {self.capacity}")
        for t in (values, labels) + (() if loss is None else (loss,)):
            if t.dtype != torch.float32 or t.device != self._ws.device or not t.is_contiguous():
                raise ValueError("ValidationMetrics: logits / scores, labels and loss must be contiguous fp32 tensors on the metrics' device")
        if int(labels.numel()) != n:
            raise ValueError(f"ValidationMetrics: {n} predictions with {int(labels.numel())} labels")
        _lib.check(fn(self._ws.data_ptr(), self.capacity, values.data_ptr(), labels.data_ptr(), 0 if loss is None else loss.data_ptr(), off, n,
                      int(n_targets), _lib.stream()))
        self.cursor = max(self.cursor, off + n)
        self.n_targets += int(n_targets)

    def update(self, logits: torch.Tensor, labels: torch.Tensor, loss: torch.Tensor = None, n_targets: int = 0, offset: int = None) -> None:
        """One validation batch: sigmoid(logits) and labels go to the next len(logits) slots (or to `offset` ..), the accumulator gains
        (double)loss * n_targets.  Enqueues one launch on the current stream; never waits for the device."""
        self._append(self.lib.pmgt_eval_append, logits, labels, loss, n_targets, offset)

    def update_scores(self, scores: torch.Tensor, labels: torch.Tensor, loss: torch.Tensor = None, n_targets: int = 0, offset: int = None) -> None:
        """`update` with ready scores (no sigmoid): predictions gathered from other ranks, and the operator tests."""
        self._append(self.lib.pmgt_op_eval_append_scores, scores, labels, loss, n_targets, offset)

    def _header(self):
        h = self._ws[:HEADER_BYTES].cpu().numpy()        # the one device-to-host copy
        return float(h[:8].view(np.float64)[0]), [int(x) for x in h.view(np.uint64)]

    def loss_sum(self) -> float:
        """sum over the updates of (double)loss * n_targets, as accumulated so far (reads the device)."""
        return self._header()[0]

    def statistic(self) -> dict:
        """Runs the reduce and returns its integers: twoU, n_pos, n_neg, nan (reads the device)."""
        if self.cursor < 1:
            raise ValueError("ValidationMetrics: no prediction was added")
        _lib.check(self.lib.pmgt_eval_reduce(self._ws.data_ptr(), self.capacity, self.cursor, _lib.stream()))
        acc, u = self._header()
        return dict(acc=acc, twoU=u[1], n_pos=u[2], n_neg=u[3], nan=u[4], n=u[5])

    def result(self) -> dict:
        st = self.statistic()
        if st["nan"]:
            raise ValueError(f"ValidationMetrics: {st['nan']} of {self.cursor} scores are NaN")
        if st["n_pos"] == 0 or st["n_neg"] == 0:
            raise ValueError(ONE_CLASS)
        return {"loss/val": float(st["acc"] / max(self.n_targets, 1)),
                "val/auc": float(st["twoU"]) / (2.0 * st["n_pos"] * st["n_neg"])}

    def scores(self) -> np.ndarray:
        lo = HEADER_BYTES + 4 * self._capr
        return self._ws[lo: lo + 4 * self.cursor].cpu().numpy().view(np.float32).copy()

    def labels(self) -> np.ndarray:
        lo = HEADER_BYTES + 8 * self._capr
        return self._ws[lo: lo + self.cursor].cpu().numpy().astype(np.float32)


RANK_HEADER_BYTES = 128       # PMGT_RANK_HEADER_BYTES
RANK_MAX_ROW, RANK_MAX_K, RANK_MAX_KS, RANK_MAX_USERS = 4096, 1024, 4, 1 << 22      # PMGT_RANK_MAX_*; the user slots of one workspace


def discount_tables(max_k: int):
    """disc[r] = 1 / log2(r + 2) and idcg = cumsum(disc) in fp64, r < max_k: `log` and `log.cumsum()` of get_ndcg (pmgt/metrics.py:19,26).
    The host path and the device path both read THESE numbers; the device evaluates no logarithm."""
    disc = 1.0 / np.log2(np.arange(int(max_k)) + 2)
    return disc, disc.cumsum()


def check_ks(ks):
    ks = tuple(int(k) for k in ks)
    if not 1 <= len(ks) <= RANK_MAX_KS or any(k < 1 or k > RANK_MAX_K for k in ks) or any(b <= a for a, b in zip(ks, ks[1:])):
        raise ValueError(f"ks={ks!r}: expected 1 to {RANK_MAX_KS} strictly increasing cut-offs in [1, {RANK_MAX_K}]")
    return ks


class RankingMetrics:
    """`max_users` user slots on `device`.  reset() -> update(...) per batch of users -> result() / per_user().  A row of `logits` holds one
    user's candidate scores, `labels` marks the positives (!= 0), `counts` the live candidates per row (None = full rows; entries past the
    count are padding).  Ranks follow the project's tie rule: among equal scores the lower candidate index ranks first.  The cursor (next
    free slot) is a host integer.  workspace: optional uint8 device tensor of at least `workspace_bytes(max_users, len(ks))` bytes."""

    def __init__(self, device, max_users: int, ks=(10, 20), workspace: torch.Tensor = None):
        self.lib = _lib.hip()
        self.device = torch.device(device)
        self.max_users = int(max_users)
        self.ks = check_ks(ks)
        self.nbytes = self.workspace_bytes(self.max_users, len(self.ks))
        if workspace is None:
            workspace = torch.empty(self.nbytes, dtype=torch.uint8, device=self.device)
        if workspace.dtype != torch.uint8 or not workspace.is_contiguous() or workspace.numel() < self.nbytes:
            raise ValueError(f"RankingMetrics: the workspace must be a contiguous uint8 tensor of >= {self.nbytes} bytes")
        self._ws = workspace
        self._capr = (self.max_users + 63) // 64 * 64
        self._ks_c = (C.c_int * len(self.ks))(*self.ks)
        self._disc, self._idcg = (np.ascontiguousarray(t) for t in discount_tables(self.ks[-1]))
        self.cursor = 0
        self.reset()

    @staticmethod
    def workspace_bytes(max_users: int, n_k: int = 2) -> int:
        n = int(_lib.hip().pmgt_rank_workspace_bytes(int(max_users), int(n_k)))
        if n < 0:
            raise ValueError(f"RankingMetrics: max_users = {max_users!r} outside [1, {RANK_MAX_USERS}] or {n_k!r} cut-offs outside [1, {RANK_MAX_KS}]")
        return n

    def reset(self) -> None:
        _lib.check(self.lib.pmgt_rank_reset(self._ws.data_ptr(), self.max_users, self._ks_c, len(self.ks), self._disc.ctypes.data,
                                            self._idcg.ctypes.data, _lib.stream()))
        self.cursor = 0

    def update(self, logits: torch.Tensor, labels: torch.Tensor, counts: torch.Tensor = None, offset: int = None) -> None:
        """One batch of users: logits and labels [n_users, C] (fp32, contiguous, on the metrics' device), counts [n_users] int32 or None.  The
        records go to the next n_users slots (or to `offset` ..; the updates of one evaluation must cover every slot below the cursor, result()
        refuses a gap).  A label other than 0 counts as 1, in the loss too.  Enqueues one launch on the current stream; never waits for the device."""
        if logits.dim() != 2 or labels.shape != logits.shape:
            raise ValueError(f"RankingMetrics: logits {tuple(logits.shape)} and labels {tuple(labels.shape)} must be one [n_users, C] shape")
        n, stride = int(logits.shape[0]), int(logits.shape[1])
        if not 1 <= stride <= RANK_MAX_ROW:
            raise ValueError(f"RankingMetrics: {stride} candidates per row outside [1, {RANK_MAX_ROW}]")
        off = self.cursor if offset is None else int(offset)
        if off < 0 or off + n > self.max_users:
            raise ValueError(f"RankingMetrics: users [{off}, {off + n}) do not fit max_users = {self.max_users}")
        for t in (logits, labels):
            if t.dtype != torch.float32 or t.device != self._ws.device or not t.is_contiguous():
                raise ValueError("RankingMetrics: logits and labels must be contiguous fp32 tensors on the metrics' device")
        if counts is not None and (counts.dtype != torch.int32 or counts.device != self._ws.device or not counts.is_contiguous()
                                   or tuple(counts.shape) != (n,)):
            raise ValueError("RankingMetrics: counts must be a contiguous int32 tensor [n_users] on the metrics' device")
        _lib.check(self.lib.pmgt_rank_append(self._ws.data_ptr(), self.max_users, logits.data_ptr(), labels.data_ptr(),
                                             0 if counts is None else counts.data_ptr(), stride, off, n, _lib.stream()))
        self.cursor = max(self.cursor, off + n)

    def statistic(self) -> dict:
        """Runs the reduce and returns the header: the sums per k, the loss sum and the three counts (reads the device)."""
        if self.cursor < 1:
            raise ValueError("RankingMetrics: no user was added")
        _lib.check(self.lib.pmgt_rank_reduce(self._ws.data_ptr(), self.max_users, self.cursor, _lib.stream()))
        h = self._ws[:RANK_HEADER_BYTES].cpu().numpy()        # the one device-to-host copy
        f, u = h.view(np.float64), h.view(np.uint64)
        return dict(ndcg={k: float(f[i]) for i, k in enumerate(self.ks)}, recall={k: float(f[RANK_MAX_KS + i]) for i, k in enumerate(self.ks)},
                    loss=float(f[2 * RANK_MAX_KS]), n_users=int(u[9]), n_nan=int(u[10]), n_empty=int(u[11]), n_unwritten=int(u[12]))

    def result(self) -> dict:
        st = self.statistic()
        if st["n_unwritten"]:      # update(offset=...) left gaps below the cursor
            raise ValueError(f"RankingMetrics: {st['n_unwritten']} of the {self.cursor} user slots below the cursor were never written")
        if st["n_nan"]:
            raise ValueError(f"RankingMetrics: {st['n_nan']} of {self.cursor} users have a NaN logit among their candidates")
        if st["n_empty"]:
            raise ValueError(f"RankingMetrics: {st['n_empty']} of {self.cursor} users have no positive candidate")
        n = float(st["n_users"])
        out = {f"n{k}": st["ndcg"][k] / n for k in self.ks}
        out.update({f"r{k}": st["recall"][k] / n for k in self.ks})
        out["loss"] = st["loss"] / n
        return out

    def per_user(self) -> dict:
        """The user records of slots 0 .. cursor as numpy arrays: ndcg[k] and recall[k] fp64, loss fp32, n_pos int32, nan / empty /
        unwritten bool (a slot no update reached since the reset holds zeros)."""
        n, capr, nk = self.cursor, self._capr, len(self.ks)
        lo = RANK_HEADER_BYTES + 48 + 2 * 8 * RANK_MAX_K
        rec = self._ws[lo: self.nbytes].cpu().numpy()
        d = rec[: 2 * nk * capr * 8].view(np.float64).reshape(2, nk, capr)
        tail = rec[2 * nk * capr * 8:]
        flags = tail[8 * capr: 12 * capr].view(np.uint32)[:n]
        return dict(ndcg={k: d[0, i, :n].copy() for i, k in enumerate(self.ks)}, recall={k: d[1, i, :n].copy() for i, k in enumerate(self.ks)},
                    loss=tail[: 4 * capr].view(np.float32)[:n].copy(), n_pos=tail[4 * capr: 8 * capr].view(np.int32)[:n].copy(),
                    nan=(flags & 1) != 0, empty=(flags & 2) != 0, unwritten=(flags & 4) != 0)
