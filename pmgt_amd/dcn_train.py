"""Training and scoring of the Deep & Cross Network on the device: the reference's click-through experiment (scripts/run_dcn.sh,
pmgt/dcn/trainer.py: item_embeddings initialised from the exported embeddings, one sampled negative per positive every epoch,
BCEWithLogitsLoss, gradient clipping at 5, AdamW, validation ROC AUC with early stopping).

  DcnGrad       pmgt_dcn_train_grad / pmgt_dcn_forward over one flat parameter buffer (two launches / one); with a dropout setting,
                pmgt_dcn_train_grad_dropout: the model in training mode, the masks drawn inside the same two launches
  DcnTrainer    every trained parameter, both embedding tables included, in one flat device buffer; step() = the gradient entry +
                ONE pmgt_op_adamw over the whole buffer (five launches); capture / replay; state_dict; with dropout_seed, a model with
                dropout: its masks come from the device {seed, step} pair that pmgt_op_adamw advances
  evaluate_ctr  logits per batch from pmgt_dcn_forward, ROC AUC of sigmoid(logit) on the device (ValidationMetrics), the mean loss
  fit_dcn       epochs of sampled pairs, validation AUC / loss, early stopping, the best parameters restored

Without dropout_seed a model with emb_dropout or dropout != 0 is refused ("dropout is not covered"); validation, evaluate_ctr and the forward
entry are eval-mode arithmetic and never drop.  The model, the layout, the masks and the numpy yardstick are stated in dcn_head.py and dcn.py;
what this training shares with the NCF head's -- ng_sample, the bases PairGrad and PairTrainer, the epoch loop fit_pairs -- lives in pair_train.py."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import DCN_MAX_PAIRS, DCN_TENSORS, DcnDropoutC, DcnHeadC  # noqa: F401
from .dcn_head import (ITEM_KEY, check_dcn_covered, check_dcn_dropout, check_dcn_p, check_dcn_pairs, dcn_dropout_masks, dcn_layout, dcn_layout_slots,  # noqa: F401
                       dcn_per_layer, decays)
from .pair_train import (PairGrad, PairTrainer, bce_with_logits_host, check_ids, check_seed, fit_pairs, ng_sample,  # noqa: F401
                         normalize_item_table, pair_trainer_options)


def _model_dims(model, dropout_ok: bool = False):
    """dropout_ok: the caller runs eval-mode arithmetic on a model a seeded DcnTrainer holds, or is that trainer"""
    if not dropout_ok:
        check_dcn_dropout(model.emb_dropout.p, model.dropout_p)
    check_dcn_covered(model.factor_num, model.deep_layers, model.cross_layers)
    return (model.factor_num, model.deep_layers, model.cross_layers, model.use_layer_norm, model.user_num, model.item_num)


def model_dropout(model):
    """(p_emb, [p of every deep layer], [p of every cross layer]) as the model's Dropout modules hold them, each checked to lie in [0, 1)."""
    p_emb = check_dcn_p(model.emb_dropout.p, "emb_dropout")
    p_deep = [check_dcn_p(layer.dropout.p, f"the dropout of deep layer {l}") for l, layer in enumerate(model.deep_net.layers)]
    p_cross = [check_dcn_p(layer.dropout.p, f"the dropout of cross layer {c}") for c, layer in enumerate(model.cross_net.layers)]
    return p_emb, p_deep, p_cross


class DcnGrad(PairGrad):
    """pmgt_dcn_train_grad over one flat parameter buffer: __call__(users, items, labels) writes `grads` whole and returns (loss [1],
    logits [n]) as device tensors; forward(users, items) is pmgt_dcn_forward -> logits [n], the same bits.  Nothing is copied to the host,
    nothing waits.  `params` and `grads` are fp32 device tensors of dcn_layout's parameter count (grads None: forward only); the workspace
    grows to the largest n seen (never inside a capture: call reserve(n) first).  The library's layout is compared with dcn_layout here.
    With `dropout` = (rng, p_emb, p_deep, p_cross) the gradient entry is pmgt_dcn_train_grad_dropout, the model in training mode: rng an
    int64 [2] device tensor {seed, step} that the kernels read at every call, the p's (one, or one per layer) in [0, 1); forward() never drops."""

    who, where, max_pairs = "dcn", "the parameters' device", DCN_MAX_PAIRS
    flat_text = "dcn: {name} must be a contiguous fp32 device tensor [{count}]"
    layout_entry, layout_name, slots = "pmgt_dcn_layout", "dcn_layout", staticmethod(dcn_layout_slots)

    def __init__(self, factor_num: int, deep_layers: int, cross_layers: int, use_layer_norm: bool, layer_norm_eps: float, user_num: int,
                 item_num: int, params, grads=None, dropout=None):
        lib = self.lib = _lib.hip()
        self.layout, self.count = dcn_layout(factor_num, deep_layers, cross_layers, use_layer_norm, user_num, item_num)
        eps = float(np.float32(layer_norm_eps))
        if not eps >= 0.0:
            raise ValueError(f"dcn: layer_norm_eps = {layer_norm_eps!r} is NaN or negative")
        super().__init__((int(factor_num), int(deep_layers), int(cross_layers), int(bool(use_layer_norm))), user_num, item_num, params, grads,
                         params.device if getattr(params, "is_cuda", False) else None)      # (None: no tensor is on it, params is refused)
        self._head = DcnHeadC(*self.shape, eps, 0, self.user_num, self.item_num, params.data_ptr(), None if grads is None else grads.data_ptr())
        self._sizing = lib.pmgt_dcn_workspace_bytes
        if grads is not None:
            self._entry = lib.pmgt_dcn_train_grad
        if dropout is not None:
            rng, p_emb, p_deep, p_cross = dropout
            rng_ptr = self._check_rng(rng)
            p_deep, p_cross = dcn_per_layer(p_deep, p_cross, self.shape[1], self.shape[2])
            self._drop = DcnDropoutC(rng_ptr, check_dcn_p(p_emb, "emb_dropout"))
            for l, p in enumerate(p_deep):
                self._drop.p_deep[l] = check_dcn_p(p, f"the dropout of deep layer {l}")
            for c, p in enumerate(p_cross):
                self._drop.p_cross[c] = check_dcn_p(p, f"the dropout of cross layer {c}")
            self._entry, self._extra = lib.pmgt_dcn_train_grad_dropout, (C.byref(self._drop),)

    def forward(self, users, items, logits=None):
        import torch
        n = self._check((users, items))
        logits = torch.empty(n, dtype=torch.float32, device=self.params.device) if logits is None else logits
        _lib.check(self.lib.pmgt_dcn_forward(C.byref(self._head), users.data_ptr(), items.data_ptr(), n, logits.data_ptr(), self._ws.data_ptr(),
                                             self._ws.numel(), _lib.stream()))
        return logits


class DcnTrainer(PairTrainer):
    """AdamW on a dcn.DCN, all on the device.  Every trained parameter -- both embedding tables, the deep net, the cross weights, the
    LayerNorms, the output layer -- moves into ONE flat fp32 buffer (dcn_layout) and the model's nn.Parameters are re-pointed at views of
    it, so model.forward and state_dict see the trained weights with no copy.  `cross_net.layers.c.bias`, which the forward never reads,
    stays an ordinary nn.Parameter outside the buffer: it gets no gradient and no step, as under the reference's optimizer, which skips
    parameters whose grad is None.  The trainer owns the gradient buffer, exp_avg, exp_avg_sq, the device step counter and the decay
    mask: a tensor decays unless its name contains "bias" (get_optimizer's rule; the LayerNorms are named layer_norm, so their weights DO
    decay).  item_init [item_num, E]: copied into item_embeddings first (the DCN-PMGT variant; normalize_item_table for
    --normalize-item-init-emb).  max_grad_norm None or 0: no clipping.
    dropout_seed=<int>: the model is trained WITH ITS DROPOUT (model.emb_dropout.p on the concatenated input, each deep layer's .dropout.p
    behind its Linear and before its LayerNorm, each cross layer's .dropout.p on x0 s_c; scripts/run_dcn.sh passes --emb-dropout 0.2).
    step() is then a TRAINING-mode step whatever model.training says (pmgt_dcn_train_grad_dropout); validation, evaluate_ctr and
    grad_fn.forward stay eval-mode.  The masks come from the project's counter-based RNG over `trainer.rng`, an int64 [2] device tensor
    {seed, step}, and `step_count` is a view of rng[1:2]: the pmgt_op_adamw call that ends every step advances the mask stream, so eager
    and replayed steps draw fresh masks with no host write.  Still five launches.  Without a seed a model with dropout is refused.
    optim, scheduler_type, num_warmup_steps, num_training_steps, nonfinite, step_log, max_skipped_in_a_row: PairTrainer's."""

    who, max_pairs = "dcn", DCN_MAX_PAIRS
    layouts_differ = "the state was saved for a model of another shape or LayerNorm setting (the layouts differ)"

    def __init__(self, model, lr: float = 1e-3, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8, max_grad_norm: float = None,
                 item_init=None, dropout_seed: int = None, optim: str = "adamw", scheduler_type: str = None,
                 num_warmup_steps: int = None, num_training_steps: int = None, nonfinite: str = None, step_log: int = 0, max_skipped_in_a_row: int = 25):
        import torch
        if dropout_seed is not None:
            check_seed(dropout_seed, "dcn")
        dims = _model_dims(model, dropout_ok=dropout_seed is not None)
        drop_p = None if dropout_seed is None else model_dropout(model)
        dev = model.user_embeddings.weight.device
        if dev.type != "cuda":
            raise ValueError("dcn: the model must be on a GPU")
        E = model.factor_num << model.deep_layers
        if item_init is not None and (not isinstance(item_init, torch.Tensor) or item_init.dtype != torch.float32
                                      or tuple(item_init.shape) != (model.item_num, E)):
            raise ValueError(f"dcn: item_init must be an fp32 tensor [{model.item_num}, {E}]")
        super().__init__(model, dev, *dcn_layout(*dims), lr, weight_decay, betas, eps, max_grad_norm, dropout_seed,
                         optim=optim, scheduler_type=scheduler_type, num_warmup_steps=num_warmup_steps,
                         num_training_steps=num_training_steps, nonfinite=nonfinite, step_log=step_log, max_skipped_in_a_row=max_skipped_in_a_row)
        named = dict(model.named_parameters())
        self._adopt(lambda key: item_init if key == ITEM_KEY and item_init is not None else named[key], lambda key: True, decays)
        self.grad_fn = DcnGrad(*dims[:4], model.layer_norm_eps, model.user_num, model.item_num, self.params, self.grads,
                               dropout=None if self.rng is None else (self.rng, *drop_p))
        model._dcn_flat = self.params                        # evaluate_ctr reads the trained parameters in place
        model._dcn_dropout_seeded = self.rng is not None     # ... and, of a model trained with its dropout, in eval mode


def _flat_of(model, dropout_ok: bool = False):
    """The flat parameter buffer a DcnTrainer gave the model, or a fresh one gathered from its parameters.  dropout_ok: the caller runs
    eval-mode arithmetic only (recommend), so a model with dropout is not refused."""
    import torch
    dims = _model_dims(model, dropout_ok=dropout_ok or bool(getattr(model, "_dcn_dropout_seeded", False)))
    layout, count = dcn_layout(*dims)
    named = dict(model.named_parameters())
    first = named[next(iter(layout))]
    base = getattr(model, "_dcn_flat", None)                 # (a DcnTrainer leaves its parameter buffer here)
    if (base is not None and tuple(base.shape) == (count,)
            and all(named[k].data_ptr() == base.data_ptr() + 4 * off for k, (off, _) in layout.items())):
        return dims, base
    flat = torch.empty(count, dtype=torch.float32, device=first.device)
    with torch.no_grad():
        for k, (off, shape) in layout.items():
            flat[off: off + int(np.prod(shape))].view(shape).copy_(named[k].detach())
    return dims, flat


def evaluate_ctr(model, users, items, labels, batch_size: int = 256, metrics: str = "device") -> dict:
    """Click-through evaluation of a dcn.DCN on labelled pairs (numpy: int64 [N], int64 [N], 0 / 1 labels [N]) -> {"auc", "loss", "n"}.
    The logits come from pmgt_dcn_forward, one call per batch of `batch_size` pairs into one device buffer; nothing is copied per batch.
    AUC is that of sigmoid(logit) in fp32, as the reference ranks it (_validation_and_test_step):
      metrics="device"  ValidationMetrics: the sigmoid, the sort and the count on the device, one small copy at the end
      metrics="host"    the scores ValidationMetrics stored, copied once, through evaluation.roc_auc_score
    and `loss` is the mean BCE-with-logits over all pairs, in float64 from the logits copied once.  Where the reference turns NaN
    predictions into 0 (np.nan_to_num), a NaN logit here raises ValueError, as fit_ncf does.  A model a DcnTrainer holds is read in
    place; another model's parameters are gathered into a flat buffer first.  Always eval-mode arithmetic: a model with dropout is
    accepted when a DcnTrainer with dropout_seed holds it (it was trained that way and is scored without masks) and refused otherwise."""
    import torch
    from .evaluation import roc_auc_score
    from .metrics import ValidationMetrics
    if metrics not in ("device", "host"):
        raise ValueError(f"evaluate_ctr: metrics={metrics!r}: expected 'device' or 'host'")
    if not 1 <= int(batch_size) <= DCN_MAX_PAIRS:
        raise ValueError(f"evaluate_ctr: batch_size = {batch_size} outside [1, {DCN_MAX_PAIRS}]")
    dims, flat = _flat_of(model)
    users, items, labels = (np.ascontiguousarray(users, dtype=np.int64), np.ascontiguousarray(items, dtype=np.int64),
                            np.ascontiguousarray(labels, dtype=np.float32))
    n = len(users)
    if n < 1 or users.ndim != 1 or items.shape != (n,) or labels.shape != (n,):
        raise ValueError(f"evaluate_ctr: users {users.shape}, items {items.shape} and labels {labels.shape} must be one [N], N >= 1")
    check_ids("users", users, model.user_num, "evaluate_ctr")
    check_ids("items", items, model.item_num, "evaluate_ctr")
    dev = flat.device
    fwd = DcnGrad(*dims[:4], model.layer_norm_eps, model.user_num, model.item_num, flat)
    users_d, items_d, labels_d = torch.from_numpy(users).to(dev), torch.from_numpy(items).to(dev), torch.from_numpy(labels).to(dev)
    logits = torch.empty(n, dtype=torch.float32, device=dev)
    vm = ValidationMetrics(dev, n)
    for lo in range(0, n, int(batch_size)):
        hi = min(lo + int(batch_size), n)
        fwd.forward(users_d[lo:hi], items_d[lo:hi], logits=logits[lo:hi])
        vm.update(logits[lo:hi], labels_d[lo:hi])
    if metrics == "device":
        auc = vm.result()["val/auc"]                         # (raises for NaN scores and for one class)
        z = logits.cpu().numpy()
    else:
        z = logits.cpu().numpy()
        if np.isnan(z).any():
            raise ValueError(f"evaluate_ctr: {int(np.isnan(z).sum())} of {n} logits are NaN")
        auc = roc_auc_score(vm.labels(), vm.scores())
    if np.isnan(z).any():
        raise ValueError(f"evaluate_ctr: {int(np.isnan(z).sum())} of {n} logits are NaN")
    return {"auc": float(auc), "loss": bce_with_logits_host(z, labels), "n": n}


def validation_seed(seed: int) -> int:
    """The seed of fit_dcn's one validation draw: seed - 1 modulo 2^32 (the epochs take seed, seed + 1, ...)."""
    return (int(seed) - 1) % (1 << 32)


def fit_dcn(model, train_pairs, valid_pairs, batch_size: int, max_epochs: int, num_ng: int = 1, max_sample_items: int = 5, seed: int = 0,
            early_criterion: str = "auc", patience: int = 10, ckpt_dir: str = None, lr: float = 1e-3, weight_decay: float = 0.0,
            betas=(0.9, 0.999), eps: float = 1e-8, max_grad_norm: float = 5.0, eval_batch_size: int = 256, item_init=None, log=None,
            dropout_seed: int = None, optim: str = "adamw", scheduler_type: str = None, scheduler_warmup: float = None, nonfinite: str = None,
            step_log: int = 0, save_last: bool = False, resume_from=None):
    """Trains `model` (a dcn.DCN on a GPU) on the interaction list `train_pairs` [(user, item)], the reference's click-through fit: every
    epoch draws ng_sample(train_pairs, num_ng, seed + epoch) and visits it in the order fit_loop.epoch_order(seed, epoch); the epoch's
    users, items and labels are uploaded once and the steps run on slices (the last batch may be short), their losses stay on the device
    and are read once per epoch.  The validation set is ng_sample(valid_pairs, num_ng=max_sample_items, validation_seed(seed)) drawn ONCE before the
    first epoch -- DCNDataset's valid mode: labelled pairs, no candidate lists -- and judged by evaluate_ctr(metrics="device").  The
    reference draws its three datasets from one global numpy stream; that order of draws is NOT reproduced (each set has a seed of its
    own), and a negative is never one of the user's items of THAT list.  early_criterion: "auc" or "loss" (EarlyStopping / BestCheckpoint
    of fit_loop.py); the best epoch's parameters are restored into the model at the end (and kept as a state_dict file in ckpt_dir when
    given).  item_init: DcnTrainer's.  dropout_seed=<int> (DcnTrainer's): a model with emb_dropout / dropout > 0 is trained with them, the
    masks a pure function of the seed and the count of steps taken; validation stays in eval mode and never drops.  Without it such a
    model is refused.
    optim, scheduler_type / scheduler_warmup (a ratio of the run's steps: pair_schedule_steps), nonfinite, step_log: PairTrainer's options,
    the reference's --optim, --scheduler-type / --scheduler-warmup and --mp-enabled; save_last, resume_from: fit_pairs' (a preempted run
    continues bit for bit from ckpt_dir/last.ckpt).
    -> the history, one dict per epoch: epoch, train_loss (mean over the steps), auc, loss, best (whether it improved)."""
    if early_criterion not in ("auc", "loss"):
        raise ValueError(f"early_criterion={early_criterion!r}: expected 'auc' or 'loss'")
    if not 1 <= int(batch_size) <= DCN_MAX_PAIRS or max_epochs < 1:
        raise ValueError(f"fit_dcn: batch_size = {batch_size} outside [1, {DCN_MAX_PAIRS}] or max_epochs = {max_epochs} below 1")
    _model_dims(model, dropout_ok=dropout_seed is not None)      # (refuses unseeded dropout and uncovered shapes before anything is drawn)
    pairs = np.asarray(train_pairs, dtype=np.int64).reshape(-1, 2)
    vpairs = np.asarray(valid_pairs, dtype=np.int64).reshape(-1, 2)
    valid = ng_sample(vpairs, model.user_num, model.item_num, max_sample_items, validation_seed(seed))
    if len(pairs) < 1:
        raise ValueError("fit_dcn: no training pair")
    check_ids("users", pairs[:, 0], model.user_num, "fit_dcn")
    check_ids("items", pairs[:, 1], model.item_num, "fit_dcn")
    trainer = DcnTrainer(model, lr=lr, weight_decay=weight_decay, betas=betas, eps=eps, max_grad_norm=max_grad_norm, item_init=item_init,
                         dropout_seed=dropout_seed,
                         **pair_trainer_options("fit_dcn", len(pairs), num_ng, batch_size, max_epochs, optim, scheduler_type,
                                                scheduler_warmup, nonfinite, step_log))

    def validate(epoch: int) -> dict:
        try:
            ev = evaluate_ctr(model, *valid, batch_size=eval_batch_size, metrics="device")
        except ValueError as e:
            raise ValueError(f"fit_dcn: epoch {epoch}: validation: {e}") from e
        return {"auc": ev["auc"], "loss": ev["loss"]}

    def checkpoint(epoch: int, row: dict) -> dict:
        return {"epoch": epoch, "state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "metrics": dict(row)}

    return fit_pairs(trainer, pairs, batch_size, max_epochs, num_ng, seed, early_criterion, patience, ckpt_dir, validate, checkpoint, log,
                     save_last=save_last, resume_from=resume_from)
