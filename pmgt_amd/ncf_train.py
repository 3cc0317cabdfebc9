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

What this training shares with the DCN's lives in pair_train.py and is re-exported here: ng_sample and normalize_item_table, the bases
PairGrad (the buffer checks, the workspace, the checked call) and PairTrainer (the buffers, step, capture / replay, the state), and the epoch
loop fit_pairs.  The head (head_layout, table_layout, the yardstick ncf_head_grad_host) is stated in ncf_head.py."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import NCF_TRAIN_MAX_PAIRS, NCF_TRAIN_TENSORS, NcfDropoutC, NcfTrainC  # noqa: F401
from .ncf_head import (HEAD_PREFIXES, LAYER_DROPOUTS, TABLE_KEY, check_head_covered, check_item_table, head_layout, head_shape,  # noqa: F401
                       head_state, layout_slots, ncf_dropout_keep, ncf_dropout_masks, ncf_head_grad_host, table_layout)
from .pair_train import (PairGrad, PairTrainer, check_dropout_p, check_pairs, check_seed, fit_pairs, ng_sample, normalize_item_table,  # noqa: F401
                         pair_trainer_options, per_layer)


class NcfHeadGrad(PairGrad):
    """pmgt_ncf_train_grad over one flat parameter buffer and one frozen table: __call__(users, items, labels) writes `grads` whole and
    returns (loss [1], logits [n]) as device tensors.  Two launches; nothing is copied to the host, nothing waits.  `params` and `grads` are
    fp32 device tensors of head_layout's parameter count; the workspace grows to the largest n seen (never inside a capture: call
    reserve(n) first).  With `table_grad`, a contiguous fp32 device tensor of the table's shape, the entry is pmgt_ncf_train_grad_table:
    d loss / d table is written whole into it as well (the table is trained); `table` and `table_grad` may be views into larger buffers.
    With `dropout` = (rng, p_emb, p_layer) the entry is pmgt_ncf_train_grad_dropout, the head in training mode: rng an int64 [2] device
    tensor {seed, step} that the kernels read at every call, p_emb and p_layer (one p or one per layer) in [0, 1)."""

    who, where, max_pairs = "ncf_train", "the table's device", NCF_TRAIN_MAX_PAIRS
    flat_text = "ncf_train: {name} must be a contiguous fp32 tensor [{count}] on the table's device"
    layout_entry, layout_name, slots = "pmgt_ncf_train_layout", "head_layout", staticmethod(layout_slots)

    def __init__(self, factor_num: int, num_layers: int, kind: str, user_num: int, table, params, grads, table_grad=None, dropout=None):
        import torch
        lib = self.lib = _lib.hip()
        self.layout, self.count = head_layout(factor_num, num_layers, kind, user_num, int(table.shape[0]) if table.dim() == 2 else 0)
        self.d = factor_num << (num_layers - 1)
        check_item_table(table, None, self.d, None, "ncf_train")
        if not table.is_contiguous():
            raise ValueError("ncf_train: the item table must be contiguous")
        super().__init__((factor_num, num_layers, _lib.NCF_KINDS.index(kind)), user_num, table.shape[0], params, grads, table.device)
        if table_grad is not None and (table_grad.dtype != torch.float32 or table_grad.device != table.device
                                       or table_grad.shape != table.shape or not table_grad.is_contiguous()):
            raise ValueError(f"ncf_train: table_grad must be a contiguous fp32 tensor {tuple(table.shape)} on the table's device")
        self.table, self.table_grad = table, table_grad
        self._head = NcfTrainC(*self.shape, 0, self.user_num, self.item_num, table.data_ptr(), params.data_ptr(), grads.data_ptr())
        if table_grad is None:
            self._sizing, self._entry, self._extra = lib.pmgt_ncf_train_workspace_bytes, lib.pmgt_ncf_train_grad, ()
        else:
            self._sizing, self._entry = lib.pmgt_ncf_train_table_workspace_bytes, lib.pmgt_ncf_train_grad_table
            self._extra = (table_grad.data_ptr(),)
        if dropout is not None:
            rng, p_emb, p_layer = dropout
            rng_ptr = self._check_rng(rng)
            p_layer = per_layer(p_layer, num_layers, LAYER_DROPOUTS, "ncf_train")
            self._drop = NcfDropoutC(rng_ptr, check_dropout_p(p_emb, "emb_dropout"))
            for i, p in enumerate(p_layer):
                self._drop.p_layer[i] = check_dropout_p(p, f"the dropout of layer {i}")
            self._entry = lib.pmgt_ncf_train_grad_dropout
            self._extra = (None if table_grad is None else table_grad.data_ptr(), C.byref(self._drop))


class NcfHeadTrainer(PairTrainer):
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
    host write.  Still five launches.  Without a seed a model with dropout is refused.
    optim, scheduler_type, num_warmup_steps, num_training_steps, nonfinite, step_log, max_skipped_in_a_row: PairTrainer's."""

    who, max_pairs = "ncf_train", NCF_TRAIN_MAX_PAIRS
    layouts_differ = "the state was saved for another head, or with the table frozen / trained the other way (the layouts differ)"

    def __init__(self, model, table, lr: float = 1e-4, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_grad_norm: float = None, train_table: bool = False, dropout_seed: int = None, optim: str = "adamw", scheduler_type: str = None,
                 num_warmup_steps: int = None, num_training_steps: int = None, nonfinite: str = None, step_log: int = 0, max_skipped_in_a_row: int = 25):
        p_emb, p_layer = model.emb_dropout.p, [layer.dropout.p for layer in model.mlp_layers]
        if dropout_seed is None and (p_emb != 0 or any(p != 0 for p in p_layer)):
            raise ValueError("ncf_train: dropout in the head is not covered without dropout_seed (pass dropout_seed=<int> to train with "
                             "emb_dropout and the layers' dropout, or set them to 0)")
        if dropout_seed is not None:
            check_seed(dropout_seed, "ncf_train")
            check_dropout_p(p_emb, "emb_dropout")
            for i, p in enumerate(p_layer):
                check_dropout_p(p, f"the dropout of layer {i}")
        check_head_covered(model.factor_num, model.num_layers, model.model)
        dev = model.mlp_user_embeddings.weight.device
        check_item_table(table, model.item_num, model.factor_num << (model.num_layers - 1), dev, "ncf_train")
        self.train_table = bool(train_table)
        dims = (model.factor_num, model.num_layers, model.model, model.user_num, model.item_num)
        super().__init__(model, dev, *(table_layout(*dims) if self.train_table else head_layout(*dims)), lr, weight_decay, betas, eps,
                         max_grad_norm, dropout_seed, optim=optim, scheduler_type=scheduler_type, num_warmup_steps=num_warmup_steps,
                         num_training_steps=num_training_steps, nonfinite=nonfinite, step_log=step_log, max_skipped_in_a_row=max_skipped_in_a_row)
        named = dict(model.named_parameters())
        self._adopt(lambda key: table if key == TABLE_KEY else named[key], lambda key: key != TABLE_KEY, lambda key: not key.endswith(".bias"))
        head_count = head_layout(*dims)[1]                  # (the whole buffer when the table is frozen)
        self.table = self.views(self.params)[TABLE_KEY] if self.train_table else table.detach().contiguous()
        self.grad_fn = NcfHeadGrad(model.factor_num, model.num_layers, model.model, model.user_num, self.table, self.params[:head_count],
                                   self.grads[:head_count], table_grad=self.views(self.grads)[TABLE_KEY] if self.train_table else None,
                                   dropout=None if self.rng is None else (self.rng, p_emb, p_layer))


def fit_ncf(model, table, train_pairs, valid, batch_size: int, max_epochs: int, num_ng: int = 1, seed: int = 0, early_criterion: str = "n20",
            patience: int = 10, ckpt_dir: str = None, lr: float = 1e-4, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8,
            max_grad_norm: float = 5.0, batch_users: int = 256, log=None, train_table: bool = False, dropout_seed: int = None,
            optim: str = "adamw", scheduler_type: str = None, scheduler_warmup: float = None, nonfinite: str = None,
            step_log: int = 0, save_last: bool = False, resume_from=None):
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
    optim, scheduler_type / scheduler_warmup (a ratio of the run's steps: pair_schedule_steps), nonfinite, step_log: PairTrainer's options,
    the reference's --optim, --scheduler-type / --scheduler-warmup and --mp-enabled; save_last, resume_from: fit_pairs' (a preempted run
    continues bit for bit from ckpt_dir/last.ckpt).
    -> the history, one dict per epoch: epoch, train_loss (mean over the steps), the five metrics, best (whether it improved)."""
    import torch
    from .evaluation import check_candidates, rank_users
    from .metrics import RankingMetrics
    if early_criterion not in ("n20", "r20", "loss"):
        raise ValueError(f"early_criterion={early_criterion!r}: expected 'n20', 'r20' or 'loss'")
    if not 1 <= int(batch_size) <= NCF_TRAIN_MAX_PAIRS or max_epochs < 1:
        raise ValueError(f"fit_ncf: batch_size = {batch_size} outside [1, {NCF_TRAIN_MAX_PAIRS}] or max_epochs = {max_epochs} below 1")
    pairs = np.asarray(train_pairs, dtype=np.int64).reshape(-1, 2)
    check_pairs(pairs[:, 0], pairs[:, 1], np.ones(len(pairs), np.float32), model.user_num, model.item_num, max_pairs=1 << 40)
    valid = check_candidates(model, *valid, "fit_ncf: validation")
    trainer = NcfHeadTrainer(model, table, lr=lr, weight_decay=weight_decay, betas=betas, eps=eps, max_grad_norm=max_grad_norm,
                             train_table=train_table, dropout_seed=dropout_seed,
                             **pair_trainer_options("fit_ncf", len(pairs), num_ng, batch_size, max_epochs, optim, scheduler_type,
                                                    scheduler_warmup, nonfinite, step_log))
    dev = trainer.params.device
    on_dev = [torch.from_numpy(a).to(dev) for a in valid]
    metrics = RankingMetrics(dev, len(valid[0]), (10, 20))

    def validate(epoch: int) -> dict:
        metrics.reset()
        rank_users(model, trainer.table, *on_dev, sink=metrics.update, batch_users=batch_users)
        st = metrics.statistic()                             # (reads the device: the epoch's one wait)
        if st["n_unwritten"] or st["n_nan"]:
            raise ValueError(f"fit_ncf: epoch {epoch}: {st['n_nan']} validation users have a NaN logit")
        # a user without a positive candidate counts 0 towards nDCG and recall here (result() would refuse them)
        row = {f"n{k}": st["ndcg"][k] / st["n_users"] for k in (10, 20)}
        row.update({f"r{k}": st["recall"][k] / st["n_users"] for k in (10, 20)})
        row["loss"] = st["loss"] / st["n_users"]
        return row

    def checkpoint(epoch: int, row: dict) -> dict:
        ckpt = {"epoch": epoch, "head": {k: v.detach().cpu() for k, v in head_state(model).items()}, "metrics": dict(row)}
        if train_table:
            ckpt[TABLE_KEY] = trainer.table.detach().cpu()
        return ckpt

    history = fit_pairs(trainer, pairs, batch_size, max_epochs, num_ng, seed, early_criterion, patience, ckpt_dir, validate, checkpoint, log,
                        save_last=save_last, resume_from=resume_from)
    if train_table:
        with torch.no_grad():
            table.copy_(trainer.table)                       # (the best epoch's: fit_pairs restored head and table, one buffer)
    return history
