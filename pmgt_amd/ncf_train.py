"""Training of the head of a PMGT_NCF over an item table: the reference's downstream experiment (scripts/run_ncf.sh,
pmgt/ncf/trainer.py:183-200 with --item-init-emb-path: the exported item embeddings as the table, `num_ng` fresh negatives per positive
every epoch, BCEWithLogitsLoss, gradient clipping, AdamW, validation on nDCG / recall with early stopping).  The table is FROZEN by default
(--freeze-item-init-emb); with train_table=True it is INITIALISED from the embeddings and TRAINED WITH THE HEAD, which is what run_ncf.sh and
every config/hpo/train_ncf_*_params.json do (pmgt/ncf/trainer.py:168-179, "freeze_item_init_emb": false).

  ng_sample            the reference's training-mode negative sampling, the same stream of draws
  normalize_item_table row-wise L2 normalisation of the exported embeddings (--normalize-item-init-emb)
  NcfHeadTrainer       the head's parameters (and the table) in one flat device buffer; step() = pmgt_ncf_train_grad or
                       pmgt_ncf_train_grad_table (two launches) + pmgt_op_adamw (three); with dropout_seed, a head with dropout:
                       pmgt_ncf_train_grad_dropout, its masks drawn from the device {seed, step} pair that pmgt_op_adamw advances
  fit_ncf              epochs of sampled pairs, ranking validation, early stopping, the best head (and table) restored

The pure-numpy part needs no GPU; the head (head_layout, table_layout, check_pairs, the yardstick ncf_head_grad_host) is stated in ncf_head.py."""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import NCF_TRAIN_MAX_PAIRS, NCF_TRAIN_TENSORS, NcfDropoutC, NcfTrainC  # noqa: F401
from .ncf_head import (HEAD_PREFIXES, TABLE_KEY, check_dropout_p, check_head_covered, check_item_table, check_pairs, head_layout,  # noqa: F401
                       head_shape, head_state, layout_slots, ncf_dropout_keep, ncf_dropout_masks, ncf_head_grad_host, table_layout)


# ---- host side: pure numpy ------------------------------------------------------------------------------------------------------------------
def ng_sample(pairs, num_user: int, num_item: int, num_ng: int, seed: int, chunk: int = 1024):
    """The training pairs of one epoch as the reference draws them (NCFDataset(pairs, ..., is_training=True).ng_sample() after
    np.random.seed(seed), pmgt/ncf/datasets.py:85-101): the positives first, in the given order, then for each positive `num_ng` negatives,
    each `RandomState(seed).randint(num_item)` redrawn while the item is one of the user's items
    -> (users int64 [P (1 + num_ng)], items int64, labels fp32).
    The draws are taken `chunk` at a time (randint(n, size=k) is the stream of k scalar calls) and handed to the open slots in order; a
    rejected draw is consumed and its slot takes the next one, so no draw is skipped or reordered."""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if len(pairs) < 1 or num_ng < 0:
        raise ValueError(f"ng_sample: {len(pairs)} pairs and num_ng = {num_ng}: expected at least one pair and num_ng >= 0")
    if pairs[:, 0].min() < 0 or pairs[:, 0].max() >= num_user or pairs[:, 1].min() < 0 or pairs[:, 1].max() >= num_item:
        raise ValueError(f"ng_sample: pairs outside [0, {num_user}) x [0, {num_item})")
    keys = np.unique(pairs[:, 0] * np.int64(num_item) + pairs[:, 1])
    if num_ng > 0 and np.bincount(keys // num_item).max() >= num_item:
        raise ValueError("ng_sample: a user holds every item: no negative exists for them")
    rs = np.random.RandomState(seed)
    slot_users = np.repeat(pairs[:, 0], num_ng)
    n_slots = len(slot_users)
    neg = np.empty(n_slots, dtype=np.int64)
    s = 0
    while s < n_slots:
        m = min(int(chunk), n_slots - s)
        draws = rs.randint(num_item, size=m).astype(np.int64)
        t = 0
        while t < m:
            k = m - t                                          # (s + k <= n_slots: s grew by at most t since the chunk began)
            cand = slot_users[s: s + k] * np.int64(num_item) + draws[t:]
            at = np.minimum(np.searchsorted(keys, cand), len(keys) - 1)
            bad = keys[at] == cand
            r = int(np.argmax(bad)) if bad.any() else k
            neg[s: s + r] = draws[t: t + r]
            s += r
            t += r + (1 if r < k else 0)                       # the rejected draw is used up
    users = np.concatenate([pairs[:, 0], slot_users])
    items = np.concatenate([pairs[:, 1], neg])
    labels = np.concatenate([np.ones(len(pairs), dtype=np.float32), np.zeros(n_slots, dtype=np.float32)])
    return users, items, labels


def normalize_item_table(table):
    """Row-wise L2 normalisation of an item table [I, d] as sklearn.preprocessing.normalize does it (what --normalize-item-init-emb applies to
    the exported embeddings, load_node_init_emb, pmgt/pmgt/utils.py:37-38): norms = sqrt(einsum("ij,ij->i", X, X)) in the table's dtype, a
    norm below 10 eps counts as 1 (sklearn's _handle_zeros_in_scale: the zero row stays zero), X / norms[:, None].  numpy in, numpy out; a torch tensor comes back as a tensor of the
    same dtype on the same device (the arithmetic runs on the host: the table is normalised once, before training)."""
    if hasattr(table, "detach"):
        import torch
        out = normalize_item_table(table.detach().cpu().numpy())
        return torch.from_numpy(out).to(table.device)
    x = np.array(table, copy=True)
    if x.ndim != 2 or x.dtype.kind != "f":
        raise ValueError(f"normalize_item_table: expected a floating-point matrix [I, d], got {x.dtype} {x.shape}")
    norms = np.sqrt(np.einsum("ij,ij->i", x, x))
    norms[norms < 10 * np.finfo(norms.dtype).eps] = 1.0
    x /= norms[:, np.newaxis]
    return x


# ---- device side ------------------------------------------------------------------------------------------------------------------------------
class NcfHeadGrad:
    """pmgt_ncf_train_grad over one flat parameter buffer and one frozen table: __call__(users, items, labels) writes `grads` whole and
    returns (loss [1], logits [n]) as device tensors.  Two launches; nothing is copied to the host, nothing waits.  `params` and `grads` are
    fp32 device tensors of head_layout's parameter count; the workspace grows to the largest n seen (never inside a capture: call
    reserve(n) first).  With `table_grad`, a contiguous fp32 device tensor of the table's shape, the entry is pmgt_ncf_train_grad_table:
    d loss / d table is written whole into it as well (the table is trained); `table` and `table_grad` may be views into larger buffers.
    With `dropout` = (rng, p_emb, p_layer) the entry is pmgt_ncf_train_grad_dropout, the head in training mode: rng an int64 [2] device
    tensor {seed, step} that the kernels read at every call, p_emb and p_layer (one p or one per layer) in [0, 1)."""

    def __init__(self, factor_num: int, num_layers: int, kind: str, user_num: int, table, params, grads, table_grad=None, dropout=None):
        import torch
        self.lib = _lib.hip()
        self.layout, self.count = head_layout(factor_num, num_layers, kind, user_num, int(table.shape[0]) if table.dim() == 2 else 0)
        self.d = factor_num << (num_layers - 1)
        check_item_table(table, None, self.d, None, "ncf_train")
        if not table.is_contiguous():
            raise ValueError("ncf_train: the item table must be contiguous")
        for name, t in (("params", params), ("grads", grads)):
            if t.dtype != torch.float32 or t.device != table.device or tuple(t.shape) != (self.count,) or not t.is_contiguous():
                raise ValueError(f"ncf_train: {name} must be a contiguous fp32 tensor [{self.count}] on the table's device")
        if table_grad is not None and (table_grad.dtype != torch.float32 or table_grad.device != table.device
                                       or table_grad.shape != table.shape or not table_grad.is_contiguous()):
            raise ValueError(f"ncf_train: table_grad must be a contiguous fp32 tensor {tuple(table.shape)} on the table's device")
        self.table, self.params, self.grads, self.table_grad = table, params, grads, table_grad
        self.shape = (factor_num, num_layers, _lib.NCF_KINDS.index(kind))
        self.user_num, self.item_num = int(user_num), int(table.shape[0])
        self._head = NcfTrainC(*self.shape, 0, self.user_num, self.item_num, table.data_ptr(), params.data_ptr(), grads.data_ptr())
        offs = (C.c_int64 * NCF_TRAIN_TENSORS)()
        count = int(self.lib.pmgt_ncf_train_layout(*self.shape, self.user_num, self.item_num, offs))
        if count != self.count or list(offs) != layout_slots(self.layout):
            raise RuntimeError("ncf_train: the library's parameter layout differs from head_layout")
        self._ws, self._ws_pairs = None, 0
        self.rng = self._drop = None
        if dropout is not None:
            rng, p_emb, p_layer = dropout
            if rng.dtype != torch.int64 or tuple(rng.shape) != (2,) or rng.device != table.device or not rng.is_contiguous():
                raise ValueError("ncf_train: the dropout rng must be a contiguous int64 tensor [2] = {seed, step} on the table's device")
            p_layer = [p_layer] * num_layers if np.isscalar(p_layer) else list(p_layer)
            if len(p_layer) != num_layers:
                raise ValueError(f"ncf_train: {len(p_layer)} layer dropouts for {num_layers} layers")
            self.rng = rng
            self._drop = NcfDropoutC(rng.data_ptr(), check_dropout_p(p_emb, "emb_dropout"))
            for i, p in enumerate(p_layer):
                self._drop.p_layer[i] = check_dropout_p(p, f"the dropout of layer {i}")

    def reserve(self, n: int) -> None:
        import torch
        if n <= self._ws_pairs:
            return
        sizing = self.lib.pmgt_ncf_train_workspace_bytes if self.table_grad is None else self.lib.pmgt_ncf_train_table_workspace_bytes
        nbytes = int(sizing(*self.shape, int(n)))
        if nbytes < 0:
            raise ValueError(f"ncf_train: n = {n} pairs outside [1, {NCF_TRAIN_MAX_PAIRS}]")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ncf_train: the workspace cannot grow inside a capture; call reserve(n) first")
        self._ws, self._ws_pairs = torch.empty(nbytes, dtype=torch.uint8, device=self.table.device), int(n)

    def __call__(self, users, items, labels, loss=None, logits=None):
        import torch
        n = int(users.shape[0])
        dev = self.table.device
        for t, dt in ((users, torch.int64), (items, torch.int64), (labels, torch.float32)):
            if t.dtype != dt or tuple(t.shape) != (n,) or t.device != dev or not t.is_contiguous():
                raise ValueError("ncf_train: users, items (int64) and labels (fp32) must be contiguous [n] tensors on the table's device")
        self.reserve(n)
        loss = torch.empty(1, dtype=torch.float32, device=dev) if loss is None else loss
        logits = torch.empty(n, dtype=torch.float32, device=dev) if logits is None else logits
        front = (C.byref(self._head), users.data_ptr(), items.data_ptr(), labels.data_ptr(), n, loss.data_ptr(), logits.data_ptr())
        if self._drop is not None:
            _lib.check(self.lib.pmgt_ncf_train_grad_dropout(*front, None if self.table_grad is None else self.table_grad.data_ptr(),
                                                            C.byref(self._drop), self._ws.data_ptr(), self._ws.numel(), _lib.stream()))
        elif self.table_grad is None:
            _lib.check(self.lib.pmgt_ncf_train_grad(*front, self._ws.data_ptr(), self._ws.numel(), _lib.stream()))
        else:
            _lib.check(self.lib.pmgt_ncf_train_grad_table(*front, self.table_grad.data_ptr(), self._ws.data_ptr(), self._ws.numel(), _lib.stream()))
        return loss, logits


class NcfHeadTrainer:
    """AdamW on the head of `model` (a PMGT_NCF) over the frozen item table `table` [item_num, d] (encode_catalogue's, or exported
    embeddings uploaded), all on the device.  The head's parameters move into ONE flat fp32 buffer and the model's nn.Parameters are
    re-pointed at views of it, so model.head, state_dict, recommend and evaluate_ranking see the trained weights with no copy.  The trainer
    owns the gradient buffer, exp_avg, exp_avg_sq and the device step counter; weights and embeddings decay, biases do not
    (pmgt/base_trainer.py get_optimizer).  max_grad_norm None or 0: no clipping.
    train_table=True: the table is a parameter, initialised from `table` (which is copied, not kept) and trained with the head.  The flat
    buffer is then table_layout's: the head, a pad up to a multiple of 8 floats, the table.  `trainer.table` is a VIEW of it -- rank_users
    and recommend(table=trainer.table) read the trained rows with no copy --, the kernel's table and table_grad pointers point into the
    flat parameters and gradients, and the one pmgt_op_adamw call over the whole buffer clips head and table by ONE global norm and steps
    both: still five launches.  The table decays like every weight (get_optimizer exempts only biases and LayerNorm).  The pad floats are 0
    in the parameters, the gradients and the moments, their decay mask is 0, and nothing writes them.
    dropout_seed=<int>: the head is trained WITH ITS DROPOUT (model.emb_dropout.p on the concatenated input and on the GMF product, each
    model.mlp_layers[i].dropout.p behind its Linear; the reference's hpo_ncf_*_params.yaml search both).  step() is then a TRAINING-mode step
    whatever model.training says -- model.head, rank_users and recommend stay what the model's mode makes them, eval for validation --, the
    masks come from the project's counter-based RNG over `trainer.rng`, an int64 [2] device tensor {seed, step}, and `step_count` is a view
    of rng[1:2]: the pmgt_op_adamw call that ends every step advances the mask stream, so eager and replayed steps draw fresh masks with no
    host write.  Still five launches.  Without a seed a model with dropout is refused."""

    def __init__(self, model, table, lr: float = 1e-4, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_grad_norm: float = None, train_table: bool = False, dropout_seed: int = None):
        import torch
        import torch.nn as nn
        p_emb, p_layer = model.emb_dropout.p, [layer.dropout.p for layer in model.mlp_layers]
        if dropout_seed is None and (p_emb != 0 or any(p != 0 for p in p_layer)):
            raise ValueError("ncf_train: dropout in the head is not covered without dropout_seed (pass dropout_seed=<int> to train with "
                             "emb_dropout and the layers' dropout, or set them to 0)")
        if dropout_seed is not None:
            if isinstance(dropout_seed, bool) or not isinstance(dropout_seed, (int, np.integer)) or not -2 ** 63 <= dropout_seed < 2 ** 63:
                raise ValueError(f"ncf_train: dropout_seed = {dropout_seed!r} must be an integer that fits int64")
            check_dropout_p(p_emb, "emb_dropout")
            for i, p in enumerate(p_layer):
                check_dropout_p(p, f"the dropout of layer {i}")
        check_head_covered(model.factor_num, model.num_layers, model.model)
        dev = model.mlp_user_embeddings.weight.device
        check_item_table(table, model.item_num, model.factor_num << (model.num_layers - 1), dev, "ncf_train")
        self.model, self.train_table = model, bool(train_table)
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), (float(betas[0]), float(betas[1])), float(eps)
        self.max_grad_norm = float(max_grad_norm or 0.0)
        dims = (model.factor_num, model.num_layers, model.model, model.user_num, model.item_num)
        self.layout, self.count = table_layout(*dims) if self.train_table else head_layout(*dims)
        self.params = torch.zeros(self.count, dtype=torch.float32, device=dev)
        self.grads = torch.zeros_like(self.params)
        self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.params), torch.zeros_like(self.params)
        self.dropout_seed = None if dropout_seed is None else int(dropout_seed)
        if self.dropout_seed is None:
            self.rng, self.step_count = None, torch.zeros(1, dtype=torch.int64, device=dev)
        else:
            self.rng = torch.tensor([self.dropout_seed, 0], dtype=torch.int64, device=dev)
            self.step_count = self.rng[1:2]                  # the optimizer's step counter IS the step of the mask stream
        self.decay = torch.zeros(self.count, dtype=torch.uint8, device=dev)
        self._scal = torch.zeros(8, dtype=torch.float32, device=dev)
        self._part = torch.zeros(1024, dtype=torch.float32, device=dev)
        named = dict(model.named_parameters())
        with torch.no_grad():
            for key, (off, shape) in self.layout.items():
                view = self.params[off: off + int(np.prod(shape))].view(shape)
                if key == TABLE_KEY:
                    view.copy_(table.detach())
                else:
                    view.copy_(named[key].detach())
                    mod = model.get_submodule(key.rsplit(".", 1)[0])
                    setattr(mod, key.rsplit(".", 1)[1], nn.Parameter(view, requires_grad=True))
                if not key.endswith(".bias"):
                    self.decay[off: off + int(np.prod(shape))] = 1
        head_count = head_layout(*dims)[1]                  # (the whole buffer when the table is frozen)
        self.table = self.views(self.params)[TABLE_KEY] if self.train_table else table.detach().contiguous()
        self.grad_fn = NcfHeadGrad(model.factor_num, model.num_layers, model.model, model.user_num, self.table, self.params[:head_count],
                                   self.grads[:head_count], table_grad=self.views(self.grads)[TABLE_KEY] if self.train_table else None,
                                   dropout=None if self.rng is None else (self.rng, p_emb, p_layer))
        self._graph = self._static = None

    def views(self, flat) -> dict:
        """{state_dict key: view of `flat`} for a buffer of the layout (params, grads, exp_avg, ...)."""
        return {k: flat[off: off + int(np.prod(shape))].view(shape) for k, (off, shape) in self.layout.items()}

    def step(self, users, items, labels, loss=None):
        """One optimizer step on the pairs (device tensors: int64 [n], int64 [n], fp32 [n]; ids inside the tables, check_pairs checks them on
        the host) -> the loss before the step as a device tensor [1].  Five launches enqueued; no host copy, no synchronisation."""
        loss, _ = self.grad_fn(users, items, labels, loss=loss, logits=self._logits(int(users.shape[0])))
        _lib.check(self.grad_fn.lib.pmgt_op_adamw(self.params.data_ptr(), self.grads.data_ptr(), self.exp_avg.data_ptr(),
                                                  self.exp_avg_sq.data_ptr(), self.decay.data_ptr(), self.count, self.lr, self.weight_decay,
                                                  self.betas[0], self.betas[1], self.eps, self.max_grad_norm, self.step_count.data_ptr(),
                                                  self._scal.data_ptr(), self._part.data_ptr(), _lib.stream()))
        return loss

    def _logits(self, n: int):
        import torch
        if getattr(self, "_logit_buf", None) is None or self._logit_buf.numel() < n:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ncf_train: buffers cannot grow inside a capture")
            self._logit_buf = torch.empty(n, dtype=torch.float32, device=self.params.device)
        return self._logit_buf[:n]

    def capture(self, n: int):
        """Captures step() on `n` pairs into a graph over static input buffers -> (users, items, labels, loss): write a batch into the first
        three, replay(), read the last.  One stream.  Every buffer is created before the capture, and one warm-up step runs eagerly on the
        zeroed static batch (the kernels are loaded outside the capture) with the parameters, the moments and the step counter put back
        afterwards: capturing leaves the trainer's state as it was."""
        import torch
        if not 1 <= int(n) <= NCF_TRAIN_MAX_PAIRS:
            raise ValueError(f"ncf_train: n = {n} pairs outside [1, {NCF_TRAIN_MAX_PAIRS}]")
        dev = self.params.device
        self._static = (torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev),
                        torch.zeros(n, dtype=torch.float32, device=dev), torch.zeros(1, dtype=torch.float32, device=dev))
        self.grad_fn.reserve(n)
        self._logits(n)
        saved = self.state_dict()
        self.step(*self._static[:3], loss=self._static[3])
        self.load_state_dict(saved)
        torch.cuda.synchronize(dev)
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            self.step(*self._static[:3], loss=self._static[3])
        return self._static

    def replay(self):
        if self._graph is None:
            raise RuntimeError("ncf_train: capture(n) comes before replay()")
        self._graph.replay()
        return self._static[3]

    def state_dict(self) -> dict:
        """The flat parameters, both moments, the step counter and the layout; a trained table is inside the parameters and named by the
        layout, so a state saved frozen is refused by a trainer that trains the table, and the other way round."""
        sd = {"params": self.params.detach().clone(), "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(),
              "step": self.step_count.clone(), "layout": {k: (off, tuple(shape)) for k, (off, shape) in self.layout.items()}}
        if self.dropout_seed is not None:                    # (with "step", the whole state of the mask stream)
            sd["dropout_seed"] = self.dropout_seed
        return sd

    def load_state_dict(self, sd: dict) -> None:
        import torch
        if {k: (off, tuple(shape)) for k, (off, shape) in self.layout.items()} != dict(sd["layout"]):
            raise ValueError("ncf_train: the state was saved for another head, or with the table frozen / trained the other way "
                             "(the layouts differ)")
        if sd.get("dropout_seed") != self.dropout_seed:
            raise ValueError(f"ncf_train: the state was saved with dropout_seed = {sd.get('dropout_seed')!r}, this trainer has "
                             f"{self.dropout_seed!r}")
        with torch.no_grad():
            self.params.copy_(sd["params"])
            self.exp_avg.copy_(sd["exp_avg"])
            self.exp_avg_sq.copy_(sd["exp_avg_sq"])
            self.step_count.copy_(sd["step"])


def fit_ncf(model, table, train_pairs, valid, batch_size: int, max_epochs: int, num_ng: int = 1, seed: int = 0, early_criterion: str = "n20",
            patience: int = 10, ckpt_dir: str = None, lr: float = 1e-4, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8,
            max_grad_norm: float = 5.0, batch_users: int = 256, log=None, train_table: bool = False, dropout_seed: int = None):
    """Trains the head of `model` on the interaction list `train_pairs` [(user, item)] over the frozen `table`, the reference's downstream
    fit: every epoch draws ng_sample(seed + epoch) and visits it in the order fit_loop.epoch_order(seed, epoch); the epoch's users, items and
    labels are uploaded once and the steps run on slices (the last batch may be short), their losses stay on the device and are read once
    per epoch.  Validation ranks `valid` = (users [U], candidates [U, C], labels [U, C], counts [U]) (datasets.ranking_candidates) with
    rank_users + RankingMetrics -> n10, n20, r10, r20, loss; early_criterion: "n20", "r20" or "loss" (EarlyStopping / BestCheckpoint of
    fit_loop.py).  The best epoch's head is restored into the model at the end (and kept as a file in ckpt_dir when given).
    train_table=True (what scripts/run_ncf.sh does: the table is initialised from the embeddings and trained with the head,
    NcfHeadTrainer(train_table=True)): validation ranks over the trained table, the best epoch's table is kept and restored with the head,
    the checkpoint file gains the key "item_table", and at the end the best table is copied back into the caller's `table` tensor IN PLACE:
    `table` IS OVERWRITTEN -- recommend(table=table) and evaluate_ranking(table=table) then read the trained rows.
    dropout_seed=<int> (NcfHeadTrainer's): a model with emb_dropout / dropout > 0 is trained with them, the masks a pure function of the
    seed and the count of steps taken; validation stays in eval mode and never drops.  Without it such a model is refused.
    -> the history, one dict per epoch: epoch, train_loss (mean over the steps), the five metrics, best (whether it improved)."""
    import torch
    from .evaluation import check_candidates, rank_users
    from .fit_loop import BestCheckpoint, EarlyStopping, epoch_order, monitor_of
    from .metrics import RankingMetrics
    if early_criterion not in ("n20", "r20", "loss"):
        raise ValueError(f"early_criterion={early_criterion!r}: expected 'n20', 'r20' or 'loss'")
    if not 1 <= int(batch_size) <= NCF_TRAIN_MAX_PAIRS or max_epochs < 1:
        raise ValueError(f"fit_ncf: batch_size = {batch_size} outside [1, {NCF_TRAIN_MAX_PAIRS}] or max_epochs = {max_epochs} below 1")
    pairs = np.asarray(train_pairs, dtype=np.int64).reshape(-1, 2)
    check_pairs(pairs[:, 0], pairs[:, 1], np.ones(len(pairs), np.float32), model.user_num, model.item_num, max_pairs=1 << 40)
    valid = check_candidates(model, *valid, "fit_ncf: validation")
    trainer = NcfHeadTrainer(model, table, lr=lr, weight_decay=weight_decay, betas=betas, eps=eps, max_grad_norm=max_grad_norm,
                             train_table=train_table, dropout_seed=dropout_seed)
    dev = trainer.params.device
    on_dev = [torch.from_numpy(a).to(dev) for a in valid]
    metrics = RankingMetrics(dev, len(valid[0]), (10, 20))
    monitor, mode = monitor_of(early_criterion)
    stopper = EarlyStopping(monitor, patience, mode)
    keeper = BestCheckpoint(ckpt_dir or "", monitor, mode)
    if ckpt_dir:
        os.makedirs(ckpt_dir, exist_ok=True)
    best_params, history = None, []
    was_training = model.training
    model.eval()
    try:
        for epoch in range(int(max_epochs)):
            users, items, labels = ng_sample(pairs, model.user_num, model.item_num, num_ng, seed + epoch)
            order = epoch_order(len(users), seed, epoch)
            users_d, items_d, labels_d = (torch.from_numpy(np.ascontiguousarray(a[order])).to(dev) for a in (users, items, labels))
            n_steps = (len(order) + batch_size - 1) // batch_size
            losses = torch.empty(n_steps, 1, dtype=torch.float32, device=dev)
            for s in range(n_steps):
                lo, hi = s * batch_size, min((s + 1) * batch_size, len(order))
                trainer.step(users_d[lo:hi], items_d[lo:hi], labels_d[lo:hi], loss=losses[s])
            metrics.reset()
            rank_users(model, trainer.table, *on_dev, sink=metrics.update, batch_users=batch_users)
            st = metrics.statistic()                             # (reads the device: the epoch's one wait)
            if st["n_unwritten"] or st["n_nan"]:
                raise ValueError(f"fit_ncf: epoch {epoch}: {st['n_nan']} validation users have a NaN logit")
            # a user without a positive candidate counts 0 towards nDCG and recall here (result() would refuse them)
            row = {"epoch": epoch, "train_loss": float(losses.double().mean().item())}
            row.update({f"n{k}": st["ndcg"][k] / st["n_users"] for k in (10, 20)})
            row.update({f"r{k}": st["recall"][k] / st["n_users"] for k in (10, 20)})
            row["loss"] = st["loss"] / st["n_users"]
            write, remove = keeper.update(epoch, row[early_criterion])
            row["best"] = write is not None
            if write is not None:
                best_params = trainer.params.detach().clone()
                if ckpt_dir:
                    ckpt = {"epoch": epoch, "head": {k: v.detach().cpu() for k, v in head_state(model).items()}, "metrics": dict(row)}
                    if train_table:
                        ckpt[TABLE_KEY] = trainer.table.detach().cpu()
                    torch.save(ckpt, write)
                    if remove and os.path.exists(remove):
                        os.remove(remove)
            history.append(row)
            if log is not None:
                log(row)
            if stopper.update(row[early_criterion], epoch):
                break
        with torch.no_grad():
            if best_params is not None:
                trainer.params.copy_(best_params)            # (head and table: one buffer)
            if train_table:
                table.copy_(trainer.table)
    finally:
        model.train(was_training)
    return history
