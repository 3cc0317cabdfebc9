"""Validation metrics kept on the device (pmgt_eval_* of include/pmgt_capi.h, kernels in ops/eval_metrics.hip): what
`_validation_and_test_step` / `_valid_and_test_epoch_end` collect and compute on the host (pmgt/pmgt/trainer.py:162-195) -- sigmoid(logits)
and labels per batch, the batch loss weighted by its size, roc_auc_score at the end -- with ONE device-to-host copy per validation.

`update` enqueues a kernel and returns; only `result`, `scores`, `labels` and `loss_sum` read from the device."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib

HEADER_BYTES = 64             # PMGT_EVAL_HEADER_BYTES
MAX_CAPACITY = 1 << 26
ONE_CLASS = "Only one class present in y_true. ROC AUC score is not defined in that case."       # roc_auc_score's text


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


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
        _lib.check(self.lib.pmgt_eval_reset(self._ws.data_ptr(), self.capacity, _stream()))
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
                      int(n_targets), _stream()))
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
        _lib.check(self.lib.pmgt_eval_reduce(self._ws.data_ptr(), self.capacity, self.cursor, _stream()))
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
