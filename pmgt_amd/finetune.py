"""Fine-tuning the pre-trained encoder TOGETHER WITH the recommendation head on the device: the paper's central experiment, the reference's
PMGT_NCF (pmgt/pmgt_ncf/models.py:15-105 on the batches of pmgt/pmgt_ncf/datasets.py: one sampled context per (user, item) pair).

  PmgtNcfTrainer     one step = pmgt_encode_train -> pmgt_op_cls_gather -> pmgt_ncf_train_grad_rows -> pmgt_op_cls_scatter ->
                     pmgt_encode_backward -> ONE pmgt_op_adamw_segments over the encoder's range(s) of the engine's buffer and the head's
                     flat buffer: one global norm, one clip coefficient, one step counter, the encoder at a learning rate of its own
                     capture_step / replay_step: the whole step as one graph
  PmgtNcfOptionsTrainer  the same trainer with PairTrainer's options -- SGD, a learning-rate schedule, the step guard --: its step ends in
                     ONE pmgt_op_step_segments instead
  finetune_batches   the batches of one epoch: ng_sample's pairs in epoch_order's order, one context per pair
  fit_pmgt_ncf       epochs of such steps, ranking validation with the CURRENT encoder, early stopping, the best encoder and head restored

The head's half of the trainer is PairTrainer's (pair_train.py): its flat buffers, the {seed, step} pair, the state."""
import ctypes as C
import math
import os

import numpy as np

from . import _lib
from ._lib import NCF_TRAIN_MAX_PAIRS
from .ncf_head import LAYER_DROPOUTS, check_head_covered, head_layout, head_state, layout_slots
from .pair_train import PairGrad, PairTrainer, check_dropout_p, check_pairs, check_seed, ng_sample, per_layer

WHO = "finetune"
PAD_FLOATS = 4      # the engine keeps every tensor 16-byte aligned: consecutive entries less than this apart are one range


class NcfRowsGrad(PairGrad):
    """pmgt_ncf_train_grad_rows over one flat parameter buffer: the head on an item row PER PAIR.  bind(x_item, d_item) names the two fp32
    [n_max, d] device buffers; __call__(users, items, labels) then reads the first n rows of x_item, writes `grads` whole and the first n
    rows of d_item, and returns (loss [1], logits [n]).  Two launches.  `dropout` = (rng, p_emb, p_layer) as NcfHeadGrad takes it."""

    who, where, max_pairs = WHO, "the model's device", NCF_TRAIN_MAX_PAIRS
    flat_text = "finetune: {name} must be a contiguous fp32 tensor [{count}] on the model's device"
    layout_entry, layout_name, slots = "pmgt_ncf_train_layout", "head_layout", staticmethod(layout_slots)

    def __init__(self, factor_num: int, num_layers: int, kind: str, user_num: int, item_num: int, params, grads, dropout=None):
        lib = self.lib = _lib.hip()
        self.layout, self.count = head_layout(factor_num, num_layers, kind, user_num, item_num)
        self.d = factor_num << (num_layers - 1)
        super().__init__((factor_num, num_layers, _lib.NCF_KINDS.index(kind)), user_num, item_num, params, grads, params.device)
        self._head = _lib.NcfTrainC(*self.shape, 0, self.user_num, self.item_num, None, params.data_ptr(), grads.data_ptr())
        self._sizing, self._entry = lib.pmgt_ncf_train_rows_workspace_bytes, lib.pmgt_ncf_train_grad_rows
        self._drop_ref = None
        if dropout is not None:
            rng, p_emb, p_layer = dropout
            rng_ptr = self._check_rng(rng)
            p_layer = per_layer(p_layer, num_layers, LAYER_DROPOUTS, WHO)
            self._drop = _lib.NcfDropoutC(rng_ptr, check_dropout_p(p_emb, "emb_dropout", WHO))
            for i, p in enumerate(p_layer):
                self._drop.p_layer[i] = check_dropout_p(p, f"the dropout of layer {i}", WHO)
            self._drop_ref = C.byref(self._drop)
        self.x_item = self.d_item = None

    def bind(self, x_item, d_item) -> None:
        import torch
        for name, t in (("x_item", x_item), ("d_item", d_item)):
            if (t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != self.d or t.device != self.params.device or not t.is_contiguous()):
                raise ValueError(f"finetune: {name} must be a contiguous fp32 tensor [n, {self.d}] on the model's device")
        self.x_item, self.d_item = x_item, d_item
        self._extra = (x_item.data_ptr(), d_item.data_ptr(), self._drop_ref)

    def __call__(self, users, items, labels, loss=None, logits=None):
        if self.x_item is None or int(users.shape[0]) > min(self.x_item.shape[0], self.d_item.shape[0]):
            raise ValueError("finetune: bind(x_item, d_item) with at least n rows comes before the call")
        return super().__call__(users, items, labels, loss=loss, logits=logits)


def encoder_segments(engine) -> list:
    """[(lo, hi)] in floats: the ranges of the engine's flat buffer that pmgt_encode_backward writes -- its `bert.*` entries, consecutive
    ones merged (the alignment pad between two tensors, below 4 floats, belongs to the range: its gradient is never written and stays 0).
    Anything else in the buffer (the NFR head of the pre-training) lies outside."""
    spans = sorted((e["offset"], e["offset"] + e["numel"]) for e in engine.entries if e["name"].startswith("bert."))
    out = []
    for lo, hi in spans:
        if out and lo - out[-1][1] < PAD_FLOATS:
            out[-1][1] = max(out[-1][1], hi)
        else:
            out.append([lo, hi])
    return [(lo, hi) for lo, hi in out]


class PmgtNcfTrainer(PairTrainer):
    """AdamW on a PMGT_NCF, ENCODER AND HEAD, all on the device.  The head's parameters move into one flat fp32 buffer exactly as
    NcfHeadTrainer moves them (the model's nn.Parameters become views; weights and embeddings decay, biases do not); the encoder's stay where
    they are, in `engine.params`, and the trainer owns a gradient buffer (`enc_grads`, the engine's layout) and both moments for every
    range of that buffer the encoder's backward writes (`segments`, encoder_segments: the `bert.*` entries; the NFR head of the
    pre-training is neither stepped nor decayed nor counted in the norm), with the engine's own decay flags.  `engine.opt_step`, the
    engine's moments and `engine.grads` are not used.
    step(users, items, labels, node_ids, attention_mask) enqueues pmgt_encode_train (TRAINING flag on: the encoder's own dropout follows
    its config and advances `engine.rng_state`), pmgt_op_cls_gather, pmgt_ncf_train_grad_rows, pmgt_op_cls_scatter, pmgt_encode_backward
    and ONE pmgt_op_adamw_segments over the encoder's range(s) at lr_scale = encoder_lr / lr and the head at 1: one global norm, one clip
    coefficient (max_grad_norm None or 0: none), one step counter -- the trainer's `step_count`; with dropout_seed it is rng[1], so the step
    that ends in it advances the head's mask stream.  No torch op, no host copy, no wait and no allocation once reserve(n, seq_len) has run.
    Every `check_carrier_every` steps, and after load_state_dict, the LayerNorm-carrier guard of the engine runs (Trainer._check_carrier's:
    the encoder's LayerNorm parameters move): one small read.
    dropout_seed=<int>: the head is trained with its dropout as NcfHeadTrainer trains it; without it a head with dropout is refused.
    An fp8 engine is REFUSED: the glue kernels read and write fp32 or bf16 activations, and fine-tuning on quantised tables is not stated
    by the reference.
    This class takes none of PairTrainer's optimizer options (its keywords are the ones it always had, and another one is a TypeError);
    PmgtNcfOptionsTrainer below is this trainer WITH them -- SGD, a learning-rate schedule, the step guard -- and everything else here,
    the skipped step and the captured step included, is written for both.
    A SKIPPED step (nonfinite="skip", a non-finite joint gradient norm) leaves engine.params -- the whole buffer --, the head, every moment
    and the step counter untouched.  The encoder's own dropout counter (engine.rng_state) HAS advanced, because the forward ran; the head's
    mask stream, which is the step counter, has not: the next step draws the head's masks again and fresh ones for the encoder.  Both
    counters move on the device as functions of what came before, so a run stays a pure function of its seeds.
    capture_step(n, seq_len) / replay_step() run the whole step as one graph; the carrier guard drops and re-captures it when it must."""

    who, max_pairs = WHO, NCF_TRAIN_MAX_PAIRS
    layouts_differ = "the state was saved for another head or another encoder (the layouts differ)"

    def __init__(self, model, lr: float = 1e-4, encoder_lr: float = None, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_grad_norm: float = None, dropout_seed: int = None, check_carrier_every: int = 200):
        self._setup(model, lr, encoder_lr, weight_decay, betas, eps, max_grad_norm, dropout_seed, check_carrier_every)

    def _setup(self, model, lr, encoder_lr, weight_decay, betas, eps, max_grad_norm, dropout_seed, check_carrier_every, **options):
        """Everything __init__ does; `options`: PairTrainer.__init__'s optimizer options (PmgtNcfOptionsTrainer states them), none here."""
        import torch
        check_head_covered(model.factor_num, model.num_layers, model.model)
        d = model.factor_num << (model.num_layers - 1)
        if model.config.hidden_size != d:
            raise ValueError(f"finetune: config.hidden_size = {model.config.hidden_size} must equal factor_num << (num_layers - 1) = {d}: "
                             "the item's CLS state is the item half of layer 0's input")
        p_emb, p_layer = model.emb_dropout.p, [layer.dropout.p for layer in model.mlp_layers]
        if dropout_seed is None and (p_emb != 0 or any(p != 0 for p in p_layer)):
            raise ValueError("finetune: dropout in the head is not covered without dropout_seed (pass dropout_seed=<int> to train with "
                             "emb_dropout and the layers' dropout, or set them to 0)")
        if dropout_seed is not None:
            check_seed(dropout_seed, WHO)
        scale = 1.0
        if encoder_lr is not None:
            if not (isinstance(encoder_lr, (int, float, np.floating)) and math.isfinite(encoder_lr) and encoder_lr >= 0):
                raise ValueError(f"finetune: encoder_lr = {encoder_lr!r} must be a finite rate >= 0")
            if not lr > 0:
                raise ValueError(f"finetune: encoder_lr is a rate relative to lr, which must be > 0 (got lr = {lr!r})")
            scale = float(encoder_lr) / float(lr)
        eng = self.engine = model.engine
        if eng.dtype_name not in ("fp32", "bf16"):
            raise ValueError(f"finetune: a {eng.dtype_name!r} engine is not covered (fp32 and bf16 are)")
        dev = eng.device
        dims = (model.factor_num, model.num_layers, model.model, model.user_num, model.item_num)
        PairTrainer.__init__(self, model, dev, *head_layout(*dims), lr, weight_decay, betas, eps, max_grad_norm, dropout_seed, **options)
        # any option set: the step ends in pmgt_op_step_segments and the state names the options; none: pmgt_op_adamw_segments and the state as ever
        self._options = self.optim != "adamw" or self.scheduler_type is not None or self._guard_state is not None
        named = dict(model.named_parameters())
        self._adopt(lambda key: named[key], lambda key: True, lambda key: not key.endswith(".bias"))
        self.encoder_lr, self.lr_scale = (self.lr if encoder_lr is None else float(encoder_lr)), scale
        self.grad_fn = NcfRowsGrad(*dims, self.params, self.grads, dropout=None if self.rng is None else (self.rng, p_emb, p_layer))
        self.d = d
        self.segments = encoder_segments(eng)
        if not 1 <= len(self.segments) < _lib.ADAM_MAX_SEGMENTS:
            raise ValueError(f"finetune: the encoder's parameters form {len(self.segments)} ranges, {_lib.ADAM_MAX_SEGMENTS - 1} at most")
        self.enc_grads = torch.zeros_like(eng.params)
        adam = self.optim == "adamw"                         # (SGD holds no moments, for head or encoder: the segments' m and v are NULL)
        self.enc_exp_avg = [torch.zeros(hi - lo, dtype=torch.float32, device=dev) for lo, hi in self.segments] if adam else []
        self.enc_exp_avg_sq = [torch.zeros_like(m) for m in self.enc_exp_avg]
        n_seg = len(self.segments) + 1
        self._segs = (_lib.AdamSegmentC * n_seg)()
        for k, (lo, hi) in enumerate(self.segments):
            self._segs[k] = _lib.AdamSegmentC(eng.params[lo:hi].data_ptr(), self.enc_grads[lo:hi].data_ptr(),
                                              self.enc_exp_avg[k].data_ptr() if adam else None,
                                              self.enc_exp_avg_sq[k].data_ptr() if adam else None, eng.decay_mask[lo:hi].data_ptr(), hi - lo,
                                              self.lr_scale)
        self._segs[n_seg - 1] = _lib.AdamSegmentC(self.params.data_ptr(), self.grads.data_ptr(), self.exp_avg.data_ptr() if adam else None,
                                                  self.exp_avg_sq.data_ptr() if adam else None, self.decay.data_ptr(), self.count, 1.0)
        self._part = torch.zeros(1024 * n_seg, dtype=torch.float32, device=dev)
        self._loss = torch.zeros(1, dtype=torch.float32, device=dev)
        self.check_carrier_every = int(check_carrier_every)
        self._steps = 0
        self._capturing = False
        self._graph_end = self._graph_keep = None
        self._rows = self._seq = 0
        self._ws = self._last = self._d_last = self._x_item = self._d_item = None

    # ---- buffers ----------------------------------------------------------------------------------------------------------------------------
    def reserve(self, n: int, seq_len: int = None) -> None:
        """Every buffer a step on up to `n` pairs with contexts of `seq_len` tokens needs (seq_len None: the length seen last, else the
        config's max_position_embeddings): the encoder's training workspace (pmgt_workspace_bytes(e, n, S, 1, 1)), the head's workspace,
        last_hidden and its gradient [n, S, d] in the engine dtype, the CLS rows and their gradient [n, d] fp32, the logits."""
        import torch
        n, S = int(n), int(seq_len or self._seq or self.engine.config.max_position_embeddings)
        if not 1 <= n <= NCF_TRAIN_MAX_PAIRS:
            raise ValueError(f"finetune: n = {n} pairs outside [1, {NCF_TRAIN_MAX_PAIRS}]")
        eng, dev = self.engine, self.params.device
        need = eng._workspace_bytes(n, S, 1, True)
        if need < 0:
            raise ValueError(f"finetune: {eng.lib.pmgt_last_error().decode()}")
        if self._ws is None or self._ws.numel() < need:
            self._ws = None
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        if n * S > self._rows * self._seq or n > self._rows:
            rows = max(n, self._rows)
            self._last = torch.empty(rows * S * self.d, dtype=eng.torch_dtype, device=dev)
            self._d_last = torch.empty_like(self._last)
            self._x_item = torch.empty(rows, self.d, dtype=torch.float32, device=dev)
            self._d_item = torch.empty_like(self._x_item)
            self.grad_fn.bind(self._x_item, self._d_item)
            self._rows, self._seq = rows, S
        self.grad_fn.reserve(n)
        self._logits(n)

    def _check_batch(self, users, items, labels, node_ids, attention_mask):
        import torch
        n = int(users.shape[0]) if isinstance(users, torch.Tensor) and users.dim() == 1 else -1
        if not 1 <= n <= NCF_TRAIN_MAX_PAIRS:
            raise ValueError(f"finetune: n = {n} pairs outside [1, {NCF_TRAIN_MAX_PAIRS}]")
        self.grad_fn._check((users, items, labels))          # (every refusal comes before the first launch: the encoder's forward moves its RNG)
        dev = self.params.device
        S = int(node_ids.shape[1]) if isinstance(node_ids, torch.Tensor) and node_ids.dim() == 2 else -1
        for t, dt in ((node_ids, torch.int64), (attention_mask, torch.float32)):
            if (not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != (n, S) or S < 1 or t.device != dev or not t.is_contiguous()):
                raise ValueError("finetune: node_ids (int64) and attention_mask (fp32) must be contiguous [n, S] tensors on the model's device, "
                                 f"n = {n} as users")
        if S > self.engine.config.max_position_embeddings:
            raise ValueError(f"finetune: S = {S} above max_position_embeddings = {self.engine.config.max_position_embeddings}")
        if self._ws is None or n > self._rows or n * S > self._rows * self._seq or self._ws.numel() < self.engine._workspace_bytes(n, S, 1, True):
            self.reserve(n, S)
        return n, S

    # ---- the step ---------------------------------------------------------------------------------------------------------------------------
    def _gradients(self, users, items, labels, node_ids, attention_mask, loss):
        """Everything of a step but the optimizer: enc_grads (the `bert.*` ranges) and the head's `grads` hold the gradients of the mean loss."""
        n, S = self._check_batch(users, items, labels, node_ids, attention_mask)
        eng, lib, st = self.engine, self.engine.lib, _lib.stream()
        loss = self._loss if loss is None else loss
        tc = eng._tensors(self.enc_grads)
        ws, nbytes, code, d = self._ws.data_ptr(), self._ws.numel(), eng.dtype_code, self.d
        flags = _lib.FLAG_TRAINING
        _lib.check(lib.pmgt_encode_train(eng.h, C.byref(tc), node_ids.data_ptr(), None, attention_mask.data_ptr(), n, S, self._last.data_ptr(),
                                         ws, nbytes, flags, st))
        _lib.check(lib.pmgt_op_cls_gather(code, self._last.data_ptr(), n, S, d, self._x_item.data_ptr(), st))
        loss, logits = self.grad_fn(users, items, labels, loss=loss, logits=self._logits(n))
        _lib.check(lib.pmgt_op_cls_scatter(code, self._d_item.data_ptr(), n, S, d, self._d_last.data_ptr(), st))
        _lib.check(lib.pmgt_encode_backward(eng.h, C.byref(tc), None, self._d_last.data_ptr(), n, S, ws, nbytes, flags, st))
        eng._raise_hook_error()
        return loss, logits

    def grad(self, users, items, labels, node_ids, attention_mask, loss=None):
        """One gradient pass without the optimizer -> (loss [1], logits [n]) as device tensors (views of the trainer's buffers); the
        gradients: encoder_grads() and views(trainer.grads).  The encoder's dropout counter advances as in a step."""
        return self._gradients(users, items, labels, node_ids, attention_mask, loss)

    def encoder_grads(self) -> dict:
        """{`bert.*` entry name: view of the trainer's encoder gradient buffer}."""
        return {e["name"]: self.enc_grads[e["offset"]: e["offset"] + e["numel"]].view(*e["shape"]) for e in self.engine.entries
                if e["name"].startswith("bert.")}

    def optimizer_step(self, loss=None) -> None:
        """The ONE clip + optimizer call over the encoder's range(s) and the head (what ends step()): pmgt_op_adamw_segments with every
        option at its default, pmgt_op_step_segments otherwise; the guard logs `loss` (None: the trainer's own loss buffer)."""
        lib, tail = self.engine.lib, (self.step_count.data_ptr(), self._scal.data_ptr(), self._part.data_ptr())
        hyper = (self.lr, self.weight_decay, self.betas[0], self.betas[1], self.eps, self.max_grad_norm)
        if self._options:
            sched, guard = self._step_options(self._loss if loss is None else loss)
            _lib.check(lib.pmgt_op_step_segments(self._segs, len(self._segs), _lib.OPTIMS.index(self.optim), *hyper, *tail, sched, guard,
                                                 _lib.stream()))
        else:
            _lib.check(lib.pmgt_op_adamw_segments(self._segs, len(self._segs), *hyper, *tail, _lib.stream()))
        if not self._capturing:                              # (a capture counts nothing and reads nothing: replay_step does)
            self._count_step()

    def _count_step(self) -> None:
        """One more step, eager or replayed; every `check_carrier_every` of them the LayerNorm-carrier guard: one small read."""
        self._steps += 1
        if self.check_carrier_every and self._steps % self.check_carrier_every == 0:
            self._check_carrier()

    def _check_carrier(self) -> None:
        """The engine's LayerNorm-carrier guard.  When it has to switch the engine to stored LayerNorm inputs while this trainer's captured
        step is alive, the graph is dropped and counted out of the engine first, and captured again over the SAME static buffers after the
        switch (the re-capture leaves the state as it was): the caller sees nothing but the engine's warning."""
        recapture = self._graph is not None and self.engine.carrier_needs_stored_inputs()
        if recapture:
            self._drop_graph()
        self.engine.check_layernorm_carrier()
        if recapture:
            self._capture()

    def step(self, users, items, labels, node_ids, attention_mask, loss=None):
        """One optimizer step on the pairs and their contexts (device tensors: users int64 [n], items int64 [n] -- 0-based item numbers,
        node_ids[:, 0] - 2 --, labels fp32 [n], node_ids int64 [n, S], attention_mask fp32 [n, S]; ids inside the tables, check_pairs checks
        them on the host) -> the loss before the step as a device tensor [1].  The launches: the encoder's forward and backward, two of
        glue, two of the head, and 2 K + 1 of the optimizer for K = len(segments) + 1 buffers."""
        loss, _ = self._gradients(users, items, labels, node_ids, attention_mask, loss)
        self.optimizer_step(loss)
        return loss

    def grad_norm(self):
        """Pre-clip global gradient norm (encoder and head) of the last step (device scalar)."""
        return self._scal[3]

    # ---- the whole step as ONE graph ----------------------------------------------------------------------------------------------------------
    def capture(self, n: int):
        raise NotImplementedError("finetune: a fine-tune step also needs the context length: capture_step(n, seq_len) / replay_step()")

    def replay(self):
        raise NotImplementedError("finetune: capture_step(n, seq_len) / replay_step() capture and replay the fine-tune step")

    def capture_step(self, n: int, seq_len: int):
        """Captures step() on `n` pairs with contexts of `seq_len` tokens into a graph over static input buffers -> (users, items, labels,
        node_ids, attention_mask, loss): write a batch into the first five, replay_step(), read the last.  One stream.  reserve(n, seq_len)
        and the LayerNorm-carrier guard run first (replays keep the kernels they were captured with); then one warm-up step runs eagerly on
        the static batch (a valid one: user 0, item 0 alone in its context) and the WHOLE state is put back -- the encoder's parameters,
        moments and dropout counter, the head, the step counter, the guard's counters and ring --, so capturing leaves the trainer as it
        was.  The engine counts the graph among its live captured steps (its options are frozen meanwhile)."""
        import torch
        n, S = int(n), int(seq_len)
        if not 1 <= S <= self.engine.config.max_position_embeddings:
            raise ValueError(f"finetune: S = {S} outside [1, max_position_embeddings = {self.engine.config.max_position_embeddings}]")
        self.reserve(n, S)
        dev = self.params.device
        self._drop_graph()
        node_ids, mask = torch.zeros(n, S, dtype=torch.int64, device=dev), torch.zeros(n, S, dtype=torch.float32, device=dev)
        node_ids[:, 0], mask[:, 0] = 2, 1.0                  # (node 2 is item 0; everything behind it is padding)
        self._static = (torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev),
                        torch.zeros(n, dtype=torch.float32, device=dev), node_ids, mask, torch.zeros(1, dtype=torch.float32, device=dev))
        self.engine.check_layernorm_carrier()
        self._capture()
        return self._static

    def _capture(self) -> None:
        """The warm-up step, the state put back, and the capture of one step over `_static`."""
        import torch
        import weakref
        n, S = self._static[3].shape
        self.reserve(n, S)                                   # (a switched option may have re-carved the encoder's workspace)
        eng, dev = self.engine, self.params.device
        saved = self.state_dict()
        self._capturing = True
        try:
            self.step(*self._static[:5], loss=self._static[5])
            self.load_state_dict(saved)
            torch.cuda.synchronize(dev)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                self.step(*self._static[:5], loss=self._static[5])
        finally:
            self._capturing = False
        eng._live_graphs += 1                                # Engine.set_option refuses changes while a captured step lives
        self._graph, self._graph_end = graph, weakref.finalize(graph, lambda: setattr(eng, "_live_graphs", eng._live_graphs - 1))
        # everything the captured launches address by raw pointer lives as long as the graph: a later, larger eager step makes reserve()
        # allocate NEW buffers and drop its references to these
        self._graph_keep = (self._ws, self._last, self._d_last, self._x_item, self._d_item, self.grad_fn._ws, self._logit_buf)

    def _drop_graph(self) -> None:
        """Forgets the captured step, if any, and counts it out of the engine's live graphs at once."""
        if self._graph is not None:
            self._graph_end()
            self._graph = self._graph_keep = None

    def replay_step(self):
        """Replays the captured step on what the static buffers hold and counts it as a step (the carrier guard's period covers eager and
        replayed steps alike, which may be mixed freely) -> the static loss buffer."""
        if self._graph is None:
            raise RuntimeError("finetune: capture_step(n, seq_len) comes before replay_step()")
        self._graph.replay()
        self._count_step()
        return self._static[5]

    # ---- state ------------------------------------------------------------------------------------------------------------------------------
    def encoder_params(self) -> list:
        """The encoder's ranges of engine.params, as views."""
        return [self.engine.params[lo:hi] for lo, hi in self.segments]

    def state_dict(self) -> dict:
        """PairTrainer's state of the head plus "encoder": the ranges, their parameters and moments (AdamW), and engine.rng_state.  With
        every option at its default the keys are the ones the state always had ("optim" and "schedule" are left out); with any option set
        it carries "optim" and "schedule", and with a guard its counters and log ring."""
        sd = super().state_dict()
        if not self._options:
            del sd["optim"], sd["schedule"]
        moments = {}
        if self.optim == "adamw":                            # (an SGD trainer holds no moments: neither key)
            moments = {"exp_avg": [m.clone() for m in self.enc_exp_avg], "exp_avg_sq": [v.clone() for v in self.enc_exp_avg_sq]}
        sd["encoder"] = {"segments": list(self.segments), "params": [p.detach().clone() for p in self.encoder_params()], **moments,
                         "rng_state": self.engine.rng_state.clone(), "dtype": self.engine.dtype_name}
        return sd

    def load_state_dict(self, sd: dict) -> None:
        """A state of other ranges, another engine dtype, layout, dropout seed, optimizer or schedule is refused before anything is written
        (a state without "optim" and "schedule" is AdamW at a constant rate)."""
        import torch
        enc = sd.get("encoder")
        if enc is None or [tuple(s) for s in enc["segments"]] != self.segments or enc.get("dtype") != self.engine.dtype_name:
            raise ValueError(f"finetune: {self.layouts_differ}")
        super().load_state_dict(sd)
        with torch.no_grad():
            for k, p in enumerate(self.encoder_params()):
                p.copy_(enc["params"][k])
            for k, (m, v) in enumerate(zip(self.enc_exp_avg, self.enc_exp_avg_sq)):
                m.copy_(enc["exp_avg"][k])
                v.copy_(enc["exp_avg_sq"][k])
            self.engine.rng_state.copy_(enc["rng_state"])
        self._check_carrier()


class PmgtNcfOptionsTrainer(PmgtNcfTrainer):
    """PmgtNcfTrainer with PairTrainer's optimizer options: optim, scheduler_type / num_warmup_steps / num_training_steps, nonfinite,
    step_log, max_skipped_in_a_row, named, meant and validated as PairTrainer.__init__ states them (the reference's --optim,
    --scheduler-type and --mp-enabled, which its fine-tune config sets).  A class of its own because PmgtNcfTrainer's keyword list is held
    to what it was (tests/test_pair_trainer_options_gpu.py); it adds the keywords and nothing else.
    With every option at its default the step and the state are PmgtNcfTrainer's, bit for bit and key for key.  With any of them set the
    step ends in ONE pmgt_op_step_segments instead of pmgt_op_adamw_segments -- the same segments, joint norm, clip and counter, under the
    schedule, the guard and AdamW or SGD; the guard logs the step's own loss --, the state carries "optim" and "schedule" and, with a guard,
    its counters and log ring, and step_log(), step_counters(), check_nonfinite() and schedule() work as inherited.  optim="sgd": no moment
    buffers exist, for head or encoder (exp_avg is None, enc_exp_avg == []), and the state has none."""

    def __init__(self, model, lr: float = 1e-4, encoder_lr: float = None, weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_grad_norm: float = None, dropout_seed: int = None, check_carrier_every: int = 200, optim: str = "adamw",
                 scheduler_type=None, num_warmup_steps=None, num_training_steps=None, nonfinite=None, step_log: int = 0,
                 max_skipped_in_a_row: int = 25):
        self._setup(model, lr, encoder_lr, weight_decay, betas, eps, max_grad_norm, dropout_seed, check_carrier_every, optim=optim,
                    scheduler_type=scheduler_type, num_warmup_steps=num_warmup_steps, num_training_steps=num_training_steps,
                    nonfinite=nonfinite, step_log=step_log, max_skipped_in_a_row=max_skipped_in_a_row)


def finetune_batches(pairs, sampler, user_num: int, item_num: int, batch_size: int, num_ng: int, seed: int, epoch: int, threads: int = 8):
    """The batches of epoch `epoch` of a fine-tuning run, a generator of (users int64 [n], items int64 [n], labels fp32 [n], node_ids int64
    [n, S], attention_mask fp32 [n, S]) numpy arrays: ng_sample(pairs, ..., seed + epoch) visited in the order
    fit_loop.epoch_order(seed, epoch), `batch_size` pairs at a time (the last batch may be short), and ONE CONTEXT PER PAIR, as the
    reference's PMGT_NCFDataset.__getitem__ samples it: node items + 2 through the sampler's inference mode, the pair at position q of the
    epoch drawing from the counter-seeded stream (seed, epoch * pairs per epoch + q).  node_ids[:, 0] == items + 2.  A pure function of
    its arguments (the sampler's own sequential stream is not touched); no GPU."""
    from .datasets import MODE_INFERENCE
    from .fit_loop import epoch_order
    if int(batch_size) < 1:
        raise ValueError(f"finetune: batch_size = {batch_size} below 1")
    users, items, labels = ng_sample(pairs, user_num, item_num, num_ng, seed + epoch)
    order = epoch_order(len(users), seed, epoch)
    users, items, labels = users[order], items[order], labels[order]
    total = len(order)
    for lo in range(0, total, int(batch_size)):
        hi = min(lo + int(batch_size), total)
        tgt = sampler.batch(items[lo:hi] + 2, MODE_INFERENCE, threads=max(int(threads), 1), base_seed=int(seed), counter=int(epoch) * total + lo)
        yield users[lo:hi], items[lo:hi], labels[lo:hi], tgt["node_ids"].numpy(), tgt["attention_mask"].numpy()


def ranking_validator(model, sampler, valid, batch_users: int, threads: int, seed: int):
    """validate(epoch) -> {n10, n20, r10, r20, loss} of fit_pmgt_ncf: the catalogue encoded with the CURRENT encoder (encode_catalogue, eval
    mode), every user's candidates ranked over that table by rank_users into a RankingMetrics; a NaN logit is refused as fit_ncf refuses it."""
    import torch
    from .evaluation import encode_catalogue, rank_users
    from .metrics import RankingMetrics
    dev = model.engine.device
    on_dev = [torch.from_numpy(a).to(dev) for a in valid]
    metrics = RankingMetrics(dev, len(valid[0]), (10, 20))

    def validate(epoch: int) -> dict:
        table = encode_catalogue(model, sampler, threads=threads, seed=seed)
        metrics.reset()
        rank_users(model, table, *on_dev, sink=metrics.update, batch_users=batch_users)
        st = metrics.statistic()                             # (reads the device: the epoch's one wait)
        if st["n_unwritten"] or st["n_nan"]:
            raise ValueError(f"fit_pmgt_ncf: epoch {epoch}: {st['n_nan']} validation users have a NaN logit")
        row = {f"n{k}": st["ndcg"][k] / st["n_users"] for k in (10, 20)}
        row.update({f"r{k}": st["recall"][k] / st["n_users"] for k in (10, 20)})
        row["loss"] = st["loss"] / st["n_users"]
        return row
    return validate


LAST_FORMAT = "pmgt_amd.fit_pmgt_ncf"      # the "format" entry of a last.ckpt fit_pmgt_ncf wrote


def fit_pmgt_ncf(model, sampler, train_pairs, valid, batch_size: int, max_epochs: int, num_ng: int = 1, seed: int = 0,
                 early_criterion: str = "n20", patience: int = 10, ckpt_dir: str = None, lr: float = 1e-4, encoder_lr: float = None,
                 weight_decay: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8, max_grad_norm: float = 5.0, dropout_seed: int = None,
                 check_carrier_every: int = 200, batch_users: int = 256, threads: int = 8, log=None, optim: str = "adamw",
                 scheduler_type=None, scheduler_warmup=None, nonfinite=None, step_log: int = 0, save_last: bool = False, resume_from=None,
                 graph: bool = False) -> list:
    """Fine-tunes `model` (a PMGT_NCF), encoder and head, on the interaction list `train_pairs` [(user, item)]: the reference's PMGT_NCF run.
    Every epoch takes PmgtNcfOptionsTrainer's steps over finetune_batches(...) -- sampled negatives, one sampled context per pair; the losses stay on
    the device and are read once per epoch -- and then validates IN EVAL MODE with the CURRENT encoder: encode_catalogue(model, sampler),
    rank_users over that table into a RankingMetrics -> n10, n20, r10, r20, loss for `valid` = (users [U], candidates [U, C], labels [U, C],
    counts [U]) (datasets.ranking_candidates).  early_criterion: "n20", "r20" or "loss" (EarlyStopping / BestCheckpoint of fit_loop.py).
    The best epoch's encoder AND head are kept on the device and restored at the end; with ckpt_dir the best file holds "bert" and "head"
    (the model's state_dict entries, on the host), "epoch" and "metrics", its predecessor removed.  The model's training / eval mode is
    restored.  The epoch loop is fit_pairs' in shape; it is restated here because a batch carries its contexts and the best state spans two
    buffers, which that loop has no place for; the run record, its comparison on resume and the atomic write are pair_train's.
    optim, scheduler_type, scheduler_warmup, nonfinite, step_log: the trainer's options as fit_ncf takes them; the schedule's lengths are
    pair_schedule_steps(len(pairs), num_ng, batch_size, max_epochs, scheduler_warmup).  With nonfinite="skip" check_nonfinite() runs once an
    epoch, after the validation -- the epoch's existing wait.
    save_last=True (needs ckpt_dir): after every epoch, and BEFORE log(row), ckpt_dir/last.ckpt is written (to a temporary name, then
    os.replace), plain data read with torch.load(weights_only=True): trainer.state_dict(), the epoch, the EarlyStopping and BestCheckpoint
    state (the best file's path in it), the best head and encoder ranges, the history, whether the run has stopped, and the call's
    batch_size, num_ng, seed, early_criterion, patience (with a schedule, max_epochs too).  resume_from=<path> or "last" restores all of
    it and continues at the next epoch; a recorded setting that differs from the call's is refused with both values named, and so is a
    file this loop did not write; a file that says the run has stopped returns its history without a step.  finetune_batches is a pure
    function of the epoch and the state holds engine.rng_state, so the resumed run is the uninterrupted one bit for bit.
    graph=True: full-size batches are copied into the static buffers of capture_step(batch_size, sampler.S) and replayed, the loss copied
    out on the device; a short last batch runs eagerly.  The history is that of graph=False bit for bit.
    -> the history, one dict per epoch: epoch, train_loss (mean over the steps), the five metrics, best (whether it improved)."""
    import torch
    from .evaluation import check_candidates
    from .fit_loop import BestCheckpoint, EarlyStopping, monitor_of
    from .pair_train import check_run_record, load_last, pair_trainer_options, run_record, save_atomic
    if early_criterion not in ("n20", "r20", "loss"):
        raise ValueError(f"early_criterion={early_criterion!r}: expected 'n20', 'r20' or 'loss'")
    if not 1 <= int(batch_size) <= NCF_TRAIN_MAX_PAIRS or max_epochs < 1:
        raise ValueError(f"fit_pmgt_ncf: batch_size = {batch_size} outside [1, {NCF_TRAIN_MAX_PAIRS}] or max_epochs = {max_epochs} below 1")
    if (save_last or resume_from == "last") and not ckpt_dir:
        raise ValueError("fit_pmgt_ncf: save_last=True and resume_from='last' need ckpt_dir")
    pairs = np.asarray(train_pairs, dtype=np.int64).reshape(-1, 2)
    check_pairs(pairs[:, 0], pairs[:, 1], np.ones(len(pairs), np.float32), model.user_num, model.item_num, max_pairs=1 << 40, who="fit_pmgt_ncf")
    valid = check_candidates(model, *valid, "fit_pmgt_ncf: validation")
    options = pair_trainer_options("fit_pmgt_ncf", len(pairs), num_ng, batch_size, max_epochs, optim=optim, scheduler_type=scheduler_type,
                                   scheduler_warmup=scheduler_warmup, nonfinite=nonfinite, step_log=step_log)
    trainer = PmgtNcfOptionsTrainer(model, lr=lr, encoder_lr=encoder_lr, weight_decay=weight_decay, betas=betas, eps=eps,
                                    max_grad_norm=max_grad_norm, dropout_seed=dropout_seed, check_carrier_every=check_carrier_every, **options)
    dev = trainer.params.device
    trainer.reserve(int(batch_size), sampler.S)
    validate = ranking_validator(model, sampler, valid, batch_users, threads, seed)
    monitor, mode = monitor_of(early_criterion)
    stopper = EarlyStopping(monitor, patience, mode)
    keeper = BestCheckpoint(ckpt_dir or "", monitor, mode)
    if ckpt_dir:
        os.makedirs(ckpt_dir, exist_ok=True)
    last_path = os.path.join(ckpt_dir, "last.ckpt") if ckpt_dir else None
    run = run_record(trainer, batch_size, num_ng, seed, early_criterion, patience, max_epochs)
    best, history, first_epoch, stopped = None, [], 0, False
    if resume_from is not None:
        ck = load_last("fit_pmgt_ncf", last_path if resume_from == "last" else resume_from, dev, LAST_FORMAT)
        check_run_record("fit_pmgt_ncf", ck["run"], run)
        trainer.load_state_dict(ck["trainer"])
        stopper.load_state_dict(ck["early_stopping"])
        keeper.load_state_dict(ck["best_checkpoint"])
        best = None if ck["best_params"] is None else (ck["best_params"], list(ck["best_encoder"]))
        history = [dict(h) for h in ck["history"]]
        first_epoch, stopped = int(ck["epoch"]) + 1, bool(ck["stopped"])
    was_training = model.training
    model.eval()
    try:
        static = trainer.capture_step(int(batch_size), sampler.S) if graph and first_epoch < int(max_epochs) and not stopped else None
        for epoch in range(first_epoch, 0 if stopped else int(max_epochs)):
            n_steps = (len(pairs) * (1 + int(num_ng)) + int(batch_size) - 1) // int(batch_size)
            losses = torch.empty(n_steps, 1, dtype=torch.float32, device=dev)
            for s, batch in enumerate(finetune_batches(pairs, sampler, model.user_num, model.item_num, batch_size, num_ng, seed, epoch,
                                                       threads=threads)):
                on_dev = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in batch]
                if static is not None and tuple(on_dev[3].shape) == tuple(static[3].shape):
                    for buf, t in zip(static, on_dev):
                        buf.copy_(t)
                    losses[s].copy_(trainer.replay_step())
                else:
                    trainer.step(*on_dev, loss=losses[s])
            metrics = validate(epoch)
            if trainer.nonfinite == "skip":
                trainer.check_nonfinite()                    # (after the epoch's one wait: the read adds none)
            row = {"epoch": epoch, "train_loss": float(losses.double().mean().item()), **metrics}
            write, remove = keeper.update(epoch, row[early_criterion])
            row["best"] = write is not None
            if write is not None:
                best = (trainer.params.detach().clone(), [p.detach().clone() for p in trainer.encoder_params()])
                if ckpt_dir:
                    sd = model.state_dict()
                    torch.save({"epoch": epoch, "bert": {k: v.detach().cpu() for k, v in sd.items() if k.startswith("bert.")},
                                "head": {k: v.detach().cpu() for k, v in head_state(model).items()}, "metrics": dict(row)}, write)
                    if remove and os.path.exists(remove):
                        os.remove(remove)
            history.append(row)
            stopped = stopper.update(row[early_criterion], epoch)      # (before log, so that last.ckpt can say it; the break still follows log)
            if save_last:
                save_atomic({"format": LAST_FORMAT, "trainer": trainer.state_dict(), "epoch": epoch, "early_stopping": stopper.state_dict(),
                             "best_checkpoint": keeper.state_dict(), "best_params": None if best is None else best[0],
                             "best_encoder": None if best is None else best[1], "history": history, "run": run, "stopped": stopped}, last_path)
            if log is not None:
                log(row)
            if stopped:
                break
        trainer._drop_graph()                                # (the restored parameters may flip the carrier: no captured step is needed any more)
        if best is not None:
            with torch.no_grad():
                trainer.params.copy_(best[0])
                for p, q in zip(trainer.encoder_params(), best[1]):
                    p.copy_(q)
            model.engine.check_layernorm_carrier()
    finally:
        trainer._drop_graph()
        model.train(was_training)
    return history
