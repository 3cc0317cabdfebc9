"""Training of the reference's stand-alone NCF model (ncf.NCF) on the device: the reference's NCF experiment (scripts/run_ncf.sh,
pmgt/ncf/trainer.py, config/hpo/*ncf*) for every kind -- MLP, GMF, NeuMF-end, NeuMF-pre -- with or without LayerNorm.

  NcfModelGrad     pmgt_ncf_model_train_grad over one flat parameter buffer (two launches); with a dropout setting, the model in
                   training mode, the masks drawn inside the same two launches
  NcfModelTrainer  every tensor the kind trains, embed_item_MLP included unless freeze_items, in one flat device buffer; step() = the
                   gradient entry + ONE pmgt_op_adamw over the whole buffer (five launches); capture / replay; state_dict
  fit_ncf_model    fit_ncf's loop: sampled pairs, ranking validation on trainer.table, early stopping, the best epoch restored

The model class is ncf.py; the layout and the numpy yardstick are stated in ncf_model.py; the bases PairGrad and PairTrainer and the epoch
loop fit_pairs live in pair_train.py.  A model without LayerNorm of kind MLP / NeuMF-end / NeuMF-pre runs the kernels of the PMGT_NCF head
(the entry hands it to them): the same bits as NcfHeadGrad on the mapped buffers."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import NCF_MODEL_KINDS, NCF_TRAIN_MAX_PAIRS, NcfDropoutC, NcfModelC
from .ncf_head import LAYER_DROPOUTS, check_item_table
from .ncf_model import ITEM_MLP, check_ncf_model_covered, ncf_model_layout, ncf_model_layout_slots, reads_mlp
from .pair_train import PairGrad, PairTrainer, check_dropout_p, check_pairs, check_seed, fit_pairs, pair_trainer_options, per_layer


def decays(key: str) -> bool:
    """get_optimizer's rule (pmgt/base_trainer.py, no_decay = ["bias", "LayerNorm.weight"]) on the NCF class's names: its LayerNorms are
    MLP_layers.{4i+2}, so their weights DO decay; a tensor decays unless its name contains "bias"."""
    return not any(nd in key for nd in ("bias", "LayerNorm.weight"))


class NcfModelGrad(PairGrad):
    """pmgt_ncf_model_train_grad over one flat parameter buffer: __call__(users, items, labels) writes `grads` whole and returns
    (loss [1], logits [n]) as device tensors.  Two launches; nothing is copied to the host, nothing waits.  `params` and `grads` are fp32
    device tensors of ncf_model_layout's count.  train_items: embed_item_MLP lies in the buffer and its gradient in `grads`; else
    `item_table`, a contiguous fp32 device tensor [item_num, d], is read and stays frozen (kind GMF reads neither).
    dropout = (rng, p_emb, p_layer): the model in training mode, NcfHeadGrad's setting."""

    who, where, max_pairs = "ncf_model", "the parameters' device", NCF_TRAIN_MAX_PAIRS
    flat_text = "ncf_model: {name} must be a contiguous fp32 device tensor [{count}]"
    layout_entry, layout_name, slots = "pmgt_ncf_model_layout", "ncf_model_layout", staticmethod(ncf_model_layout_slots)

    def __init__(self, factor_num: int, num_layers: int, kind: str, use_layer_norm: bool, layer_norm_eps: float, user_num: int, item_num: int,
                 params, grads, train_items: bool = True, item_table=None, dropout=None):
        lib = self.lib = _lib.hip()
        check_ncf_model_covered(factor_num, num_layers, kind, layer_norm_eps)
        mlp = reads_mlp(kind)
        train_items = bool(train_items) and mlp
        self.layout, self.count = ncf_model_layout(factor_num, num_layers, kind, use_layer_norm, user_num, item_num, train_items)
        dev = params.device if getattr(params, "is_cuda", False) else None      # (None: no tensor is on it, params is refused)
        super().__init__((int(factor_num), int(num_layers), NCF_MODEL_KINDS.index(kind), int(bool(use_layer_norm)), int(train_items)), user_num,
                         item_num, params, grads, dev)
        if grads is None:
            raise ValueError("ncf_model: grads is needed (there is no forward-only entry)")
        d = factor_num << (num_layers - 1)
        table_ptr = grad_ptr = None
        if train_items:
            off = self.layout[ITEM_MLP][0]
            table_ptr, grad_ptr = params.data_ptr() + 4 * off, grads.data_ptr() + 4 * off
        elif mlp:
            check_item_table(item_table, self.item_num, d, dev, "ncf_model")
            if not item_table.is_contiguous():
                raise ValueError("ncf_model: the item table must be contiguous")
            self.item_table, table_ptr = item_table, item_table.data_ptr()
        self._head = NcfModelC(*self.shape[:4], float(np.float32(layer_norm_eps)), self.shape[4], self.user_num, self.item_num, table_ptr,
                               params.data_ptr(), grads.data_ptr(), grad_ptr)
        self._sizing, self._entry, self._extra = lib.pmgt_ncf_model_workspace_bytes, lib.pmgt_ncf_model_train_grad, (None,)
        if dropout is not None:
            rng, p_emb, p_layer = dropout
            rng_ptr = self._check_rng(rng)
            p_layer = per_layer(p_layer, num_layers, LAYER_DROPOUTS, "ncf_model")
            self._drop = NcfDropoutC(rng_ptr, check_dropout_p(p_emb, "emb_dropout", "ncf_model"))
            for i, p in enumerate(p_layer):
                self._drop.p_layer[i] = check_dropout_p(p, f"the dropout of layer {i}", "ncf_model")
            self._extra = (C.byref(self._drop),)


def model_dropout(model):
    """(p_emb, [p of every layer]) as the model's Dropout modules hold them; kind GMF reads no layer, so its layers' p count as 0."""
    import torch.nn as nn
    p_layer = [m.p for m in model.MLP_layers if isinstance(m, nn.Dropout)]
    return model.emb_dropout.p, p_layer if reads_mlp(model.model) else [0.0] * len(p_layer)


class NcfModelTrainer(PairTrainer):
    """AdamW on an ncf.NCF, all on the device.  The tensors the model's kind trains move into ONE flat fp32 buffer (ncf_model_layout) and
    the model's nn.Parameters are re-pointed at views of it, so model.forward, model.head and state_dict see the trained weights with no
    copy.  `trainer.table` is the view of embed_item_MLP.weight; with freeze_items (the reference's --freeze-item-init-emb) it is a
    detached copy that stays outside the buffer and gets no step.  Tensors the kind never reads -- the GMF tables for "MLP", the MLP tables
    and layers for "GMF", every GMF_model.* / MLP_model.* of a NeuMF-pre -- stay ordinary parameters outside the buffer and keep their
    bits: they get no gradient, and the reference's AdamW skips parameters without one.  A tensor decays unless its name contains "bias"
    or "LayerNorm.weight" (get_optimizer's rule: under this class's names the LayerNorm gammas MLP_layers.{4i+2}.weight DO decay).
    max_grad_norm None or 0: no clipping.  dropout_seed=<int>: the model is trained WITH ITS DROPOUT (emb_dropout on the concatenated
    input and on the GMF product, each layer's Dropout behind its Linear and before its LayerNorm), NcfHeadTrainer's mask stream; without
    a seed a model with dropout is refused.  step, capture / replay and the state are PairTrainer's, and so are optim, scheduler_type,
    num_warmup_steps, num_training_steps, nonfinite, step_log and max_skipped_in_a_row."""

    who, max_pairs = "ncf_model", NCF_TRAIN_MAX_PAIRS
    layouts_differ = "the state was saved for another model, or with the items frozen / trained the other way (the layouts differ)"

    def __init__(self, model, lr: float = 1e-4, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8, max_grad_norm: float = None,
                 freeze_items: bool = False, dropout_seed: int = None, optim: str = "adamw", scheduler_type: str = None,
                 num_warmup_steps: int = None, num_training_steps: int = None, nonfinite: str = None, step_log: int = 0, max_skipped_in_a_row: int = 25):
        p_emb, p_layer = model_dropout(model)
        if dropout_seed is None and (p_emb != 0 or any(p != 0 for p in p_layer)):
            raise ValueError("ncf_model: dropout in the model is not covered without dropout_seed (pass dropout_seed=<int> to train with "
                             "emb_dropout and the layers' dropout, or set them to 0)")
        if dropout_seed is not None:
            check_seed(dropout_seed, "ncf_model")
            check_dropout_p(p_emb, "emb_dropout", "ncf_model")
            for i, p in enumerate(p_layer):
                check_dropout_p(p, f"the dropout of layer {i}", "ncf_model")
        check_ncf_model_covered(model.factor_num, model.num_layers, model.model, model.layer_norm_eps)
        dev = model.predict_layer.weight.device
        if dev.type != "cuda":
            raise ValueError("ncf_model: the model must be on a GPU")
        mlp = reads_mlp(model.model)
        self.train_items = mlp and not freeze_items
        dims = (model.factor_num, model.num_layers, model.model, model.use_layer_norm, model.user_num, model.item_num)
        super().__init__(model, dev, *ncf_model_layout(*dims, self.train_items), lr, weight_decay, betas, eps, max_grad_norm, dropout_seed,
                         optim=optim, scheduler_type=scheduler_type, num_warmup_steps=num_warmup_steps,
                         num_training_steps=num_training_steps, nonfinite=nonfinite, step_log=step_log, max_skipped_in_a_row=max_skipped_in_a_row)
        named = dict(model.named_parameters())
        self._adopt(lambda key: named[key], lambda key: True, decays)
        self.table = self.views(self.params)[ITEM_MLP] if self.train_items else model.embed_item_MLP.weight.detach().clone().contiguous()
        self.grad_fn = NcfModelGrad(*dims[:4], model.layer_norm_eps, model.user_num, model.item_num, self.params, self.grads,
                                    train_items=self.train_items, item_table=None if self.train_items or not mlp else self.table,
                                    dropout=None if self.rng is None else (self.rng, p_emb, p_layer))


def fit_ncf_model(model, train_pairs, valid, batch_size: int, max_epochs: int, num_ng: int = 4, seed: int = 0, early_criterion: str = "n20",
                  patience: int = 10, ckpt_dir: str = None, lr: float = 1e-4, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8,
                  max_grad_norm: float = 5.0, batch_users: int = 256, log=None, freeze_items: bool = False, dropout_seed: int = None,
                  item_init=None, optim: str = "adamw", scheduler_type: str = None, scheduler_warmup: float = None, nonfinite: str = None,
                  step_log: int = 0, save_last: bool = False, resume_from=None):
    """Trains `model` (an ncf.NCF on a GPU) on the interaction list `train_pairs` [(user, item)], fit_ncf's loop: every epoch draws
    ng_sample(seed + epoch) and visits it in the order fit_loop.epoch_order(seed, epoch); validation ranks `valid` = (users [U], candidates
    [U, C], labels [U, C], counts [U]) with rank_users + RankingMetrics on trainer.table -> n10, n20, r10, r20, loss; early_criterion:
    "n20", "r20" or "loss"; the best epoch's parameters are restored into the model at the end.  With ckpt_dir the best epoch's file holds
    {"epoch", "state_dict", "metrics"}: model.state_dict() under the reference's keys, which NCF(...).load_state_dict(..., strict=True)
    loads.  item_init [item_num, d]: exported item embeddings copied into embed_item_MLP first (--item-init-emb-path); refused unless the
    kind is MLP or NeuMF-end, as in the reference's check_args.  freeze_items, dropout_seed: NcfModelTrainer's.  A trained GMF and a
    trained MLP model then construct a NeuMF-pre: NCF(..., model="NeuMF-pre", GMF_model=gmf, MLP_model=mlp).
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
        raise ValueError(f"fit_ncf_model: batch_size = {batch_size} outside [1, {NCF_TRAIN_MAX_PAIRS}] or max_epochs = {max_epochs} below 1")
    if item_init is not None:
        d = model.factor_num << (model.num_layers - 1)
        if model.model not in ("MLP", "NeuMF-end"):
            raise ValueError(f"fit_ncf_model: item_init needs model kind 'MLP' or 'NeuMF-end', not {model.model!r}")
        if not isinstance(item_init, torch.Tensor) or item_init.dtype != torch.float32 or tuple(item_init.shape) != (model.item_num, d):
            raise ValueError(f"fit_ncf_model: item_init must be an fp32 tensor [{model.item_num}, {d}]")
    pairs = np.asarray(train_pairs, dtype=np.int64).reshape(-1, 2)
    check_pairs(pairs[:, 0], pairs[:, 1], np.ones(len(pairs), np.float32), model.user_num, model.item_num, max_pairs=1 << 40, who="fit_ncf_model")
    valid = check_candidates(model, *valid, "fit_ncf_model: validation")
    if item_init is not None:
        with torch.no_grad():
            model.embed_item_MLP.weight.copy_(item_init)
    trainer = NcfModelTrainer(model, lr=lr, weight_decay=weight_decay, betas=betas, eps=eps, max_grad_norm=max_grad_norm,
                              freeze_items=freeze_items, dropout_seed=dropout_seed,
                              **pair_trainer_options("fit_ncf_model", len(pairs), num_ng, batch_size, max_epochs, optim, scheduler_type,
                                                     scheduler_warmup, nonfinite, step_log))
    dev = trainer.params.device
    on_dev = [torch.from_numpy(a).to(dev) for a in valid]
    metrics = RankingMetrics(dev, len(valid[0]), (10, 20))

    def validate(epoch: int) -> dict:
        metrics.reset()
        rank_users(model, trainer.table, *on_dev, sink=metrics.update, batch_users=batch_users)
        st = metrics.statistic()                             # (reads the device: the epoch's one wait)
        if st["n_unwritten"] or st["n_nan"]:
            raise ValueError(f"fit_ncf_model: epoch {epoch}: {st['n_nan']} validation users have a NaN logit")
        row = {f"n{k}": st["ndcg"][k] / st["n_users"] for k in (10, 20)}
        row.update({f"r{k}": st["recall"][k] / st["n_users"] for k in (10, 20)})
        row["loss"] = st["loss"] / st["n_users"]
        return row

    def checkpoint(epoch: int, row: dict) -> dict:
        return {"epoch": epoch, "state_dict": {k: v.detach().cpu() for k, v in model.state_dict().items()}, "metrics": dict(row)}

    return fit_pairs(trainer, pairs, batch_size, max_epochs, num_ng, seed, early_criterion, patience, ckpt_dir, validate, checkpoint, log,
                     save_last=save_last, resume_from=resume_from)
