"""How a model is trained on (user, item, label) pairs on the device, stated once for the two pair heads -- the NCF head (ncf_head.py,
ncf_train.py) and the Deep & Cross Network (dcn_head.py, dcn_train.py):

  host side, numpy   ng_sample, normalize_item_table, check_ids, check_pairs, head_weights, bce_with_logits_host, and the one RNG of every
                     kernel: check_dropout_p, dropout_keep, dropout_scale, per_layer, check_seed
  PairGrad           a gradient entry over one flat parameter buffer: the buffer and layout checks, the workspace, the checked inputs
  host side, numpy   sgd_step_host (the yardstick of pmgt_op_sgd), pair_schedule_steps (the schedule's lengths of a fit_* run)
  PairTrainer        the flat buffers of the optimizer, the {seed, step} tensor, step() = the gradient entry + ONE fused optimizer entry
                     (AdamW or SGD, optionally under a learning-rate schedule and the step guard), capture / replay, the state
  fit_pairs          the epoch loop: sampled pairs, steps on slices, validation, early stopping, the best parameters kept and restored,
                     last.ckpt and the bit-identical resume

finetune.py builds on the same two bases for the NCF head that is trained TOGETHER WITH the encoder (PairGrad over the per-pair rows entry,
PairTrainer for the head's half of the buffers and of the state); its step and its epoch loop are its own.
Every refusal speaks in the name of the head that asked (`who`: "ncf_train", "dcn", "finetune").  torch is imported inside functions: importing this
loads no GPU library."""
import ctypes as C
import os

import numpy as np

from . import _lib
from ._lib import NCF_TRAIN_MAX_PAIRS


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


def check_ids(what: str, ids: np.ndarray, limit: int, who: str) -> None:
    """ValueError in the name of `who` when an id of `ids` (`what`: "users", ...) lies outside [0, limit): the kernels read by them unchecked."""
    if ids.size and (ids.min() < 0 or ids.max() >= limit):
        raise ValueError(f"{who}: {what} in [{int(ids.min())}, {int(ids.max())}] outside [0, {limit})")


def check_pairs(users, items, labels, user_num: int, item_num: int, max_pairs: int = NCF_TRAIN_MAX_PAIRS, who: str = "ncf_train"):
    """(users int64 [n], items int64 [n], labels fp32 [n]) as the kernels read them; ValueError in the name of `who` for shapes that differ,
    n outside [1, max_pairs] and ids outside the tables."""
    users, items = np.ascontiguousarray(users, dtype=np.int64), np.ascontiguousarray(items, dtype=np.int64)
    labels = np.ascontiguousarray(labels, dtype=np.float32)
    n = len(users)
    if users.ndim != 1 or items.shape != (n,) or labels.shape != (n,):
        raise ValueError(f"{who}: users {users.shape}, items {items.shape} and labels {labels.shape} must be one [n]")
    if not 1 <= n <= max_pairs:
        raise ValueError(f"{who}: n = {n} pairs outside [1, {max_pairs}]")
    check_ids("users", users, user_num, who)
    check_ids("items", items, item_num, who)
    return users, items, labels


def head_weights(weights: dict, dtype) -> dict:
    """`weights` (arrays or CPU tensors keyed like the model's state_dict; None entries dropped) as numpy arrays of `dtype`."""
    return {k: np.asarray(v.detach().cpu().numpy() if hasattr(v, "detach") else v).astype(dtype) for k, v in weights.items() if v is not None}


def bce_with_logits_host(logits: np.ndarray, labels: np.ndarray) -> float:
    """The mean of max(z, 0) - z y + log1p(exp(-|z|)) in float64."""
    z, y = np.asarray(logits, dtype=np.float64), np.asarray(labels, dtype=np.float64)
    return float((np.maximum(z, 0) - z * y + np.log1p(np.exp(-np.abs(z)))).mean())


def _fmix32(h: int) -> int:
    """The murmur3 finaliser (fmix32 of csrc/common.h) on a Python int."""
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def check_dropout_p(p, what: str, who: str = "ncf_train") -> float:
    """`p` as the fp32 value the kernels take; ValueError unless it lies in [0, 1) (a NaN does not)."""
    q = float(np.float32(p))
    if not 0.0 <= q < 1.0:
        raise ValueError(f"{who}: {what} = {p!r} outside [0, 1)")
    return q


def per_layer(p, count: int, what: str, who: str) -> list:
    """One p per layer: a scalar is repeated `count` times, a sequence must have `count` entries; if not, the refusal is `what`, which may
    leave "{}" for the numbers of entries and of layers."""
    p = [p] * count if np.isscalar(p) else list(p)
    if len(p) != count:
        raise ValueError(f"{who}: " + what.format(len(p), count))
    return p


def check_seed(seed, who: str) -> int:
    """A dropout seed as the int the device {seed, step} pair holds; ValueError unless it is an integer that fits int64."""
    if isinstance(seed, bool) or not isinstance(seed, (int, np.integer)) or not -2 ** 63 <= seed < 2 ** 63:
        raise ValueError(f"{who}: dropout_seed = {seed!r} must be an integer that fits int64")
    return int(seed)


def dropout_keep(seed: int, step: int, site: int, rows: int, cols: int, p: float) -> np.ndarray:
    """bool [rows, cols]: True where the kernels keep element (row, col) of dropout site `site` (make_drop_key and drop_keep4 of
    csrc/common.h restated in uint32 arithmetic, bit for bit; what pmgt_op_dropout_keep writes).  seed / step: the int64 values of the
    device {seed, step} pair.  One hash pair (x, y) decides the 4 columns of group col >> 2 with 16 bits each; an element is kept when its
    16 bits are >= thr >> 16, thr = (uint32)(double(float32 p) 2^32) saturated.  p = 0 keeps everything."""
    p = check_dropout_p(p, "p")
    if not p > 0.0:
        return np.ones((rows, cols), dtype=bool)
    seed, step, site = int(seed) & 0xFFFFFFFFFFFFFFFF, int(step) & 0xFFFFFFFFFFFFFFFF, int(site) & 0xFFFFFFFF
    k0 = _fmix32((seed & 0xFFFFFFFF) ^ ((site * 0x9E3779B1) & 0xFFFFFFFF))
    k1 = _fmix32((seed >> 32) + (step & 0xFFFFFFFF) * 0x7FEB352D + (step >> 32) + site)
    t = p * 4294967296.0
    thr = 0xFFFFFFFF if t >= 4294967295.0 else int(t)
    u32 = np.uint32
    r, cg = np.arange(rows, dtype=u32)[:, None], np.arange((cols + 3) // 4, dtype=u32)[None, :]
    with np.errstate(over="ignore"):
        x = r * u32(0x9E3779B1) + cg * u32(0x85EBCA77) + u32(k0)
        x ^= x >> u32(15)
        x *= u32(0x2C1B3C6D)
        x ^= x >> u32(12)
        y = x * u32(0x297A2D39) + u32(k1)
        y ^= y >> u32(15)
    lanes = np.stack([x & u32(0xFFFF), x >> u32(16), y & u32(0xFFFF), y >> u32(16)], axis=2)
    return (lanes >= u32(thr >> 16)).reshape(rows, -1)[:, :cols]


def dropout_scale(p: float) -> np.float32:
    """What a kept element is multiplied by: the fp32 value 1 / (1 - p)."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def sgd_step_host(p, g, decay, clip=None, lr_t=None, wd=0.0, dtype=np.float32, max_norm=None, lr=None, lam=None, step: int = 0):
    """pmgt_op_sgd's update on the host -> the new parameters, an array of `dtype`: per element gc = g clip; d = gc + wd p where the decay
    byte is set, else gc; p - lr_t d, every product and sum rounded to `dtype` in that order (torch.optim.SGD without momentum, coupled decay).
    dtype=np.float32 with the device's scal[0] and scal[4] as `clip` and `lr_t`: the kernel's bits.
    clip=None (the fp64 form, dtype=np.float64): the clip is computed here as clip_grad_norm_ does, min(max_norm / (norm + 1e-6), 1) for
    max_norm > 0 and 1 otherwise, and lr_t = lr * lam(step) (lam None: lr), `step` the optimizer steps completed so far."""
    p, g = np.asarray(p, dtype=dtype), np.asarray(g, dtype=dtype)
    decay = np.asarray(decay).astype(bool)
    if clip is None:
        norm = np.sqrt((g * g).sum(dtype=dtype))
        clip = min(float(max_norm) / (float(norm) + 1e-6), 1.0) if max_norm and max_norm > 0 else 1.0
        lr_t = float(lr) * (1.0 if lam is None else lam(int(step)))
    clip, lr_t, wd = dtype(clip), dtype(lr_t), dtype(wd)
    gc = g * clip
    d = np.where(decay, gc + wd * p, gc)
    return (p - lr_t * d).astype(dtype, copy=False)


def pair_schedule_steps(n_positive: int, num_ng: int, batch_size: int, max_epochs: int, scheduler_warmup=None):
    """(num_training_steps, num_warmup_steps) of a fit_pairs run: ceil(P (1 + num_ng) / batch_size) steps an epoch, times max_epochs;
    warm-up = int(scheduler_warmup * total), 0 for None.  get_scheduler of pmgt/base_trainer.py:71-90 with accumulation_step = 1 and the
    epoch's actual number of rows where the reference reads `train_ids`."""
    rows = int(n_positive) * (1 + int(num_ng))
    total = (rows + int(batch_size) - 1) // int(batch_size) * int(max_epochs)
    return total, (0 if scheduler_warmup is None else int(scheduler_warmup * total))


def pair_trainer_options(who: str, n_positive: int, num_ng: int, batch_size: int, max_epochs: int, optim="adamw", scheduler_type=None,
                         scheduler_warmup=None, nonfinite=None, step_log: int = 0) -> dict:
    """The PairTrainer keywords of a fit_* call: its options as they are, the schedule's lengths from pair_schedule_steps."""
    if scheduler_type is None and scheduler_warmup is not None:
        raise ValueError(f"{who}: scheduler_warmup = {scheduler_warmup!r} without scheduler_type")
    opts = dict(optim=optim, nonfinite=nonfinite, step_log=step_log)
    if scheduler_type is not None:
        total, warmup = pair_schedule_steps(n_positive, num_ng, batch_size, max_epochs, scheduler_warmup)
        opts.update(scheduler_type=scheduler_type, num_warmup_steps=warmup, num_training_steps=total)
    return opts


# ---- device side ------------------------------------------------------------------------------------------------------------------------------
class PairGrad:
    """A gradient entry of the library over one flat parameter buffer: __call__(users, items, labels) writes `grads` whole and returns
    (loss [1], logits [n]) as device tensors.  Two launches; nothing is copied to the host, nothing waits.  The workspace grows to the
    largest n seen (never inside a capture: call reserve(n) first).
    A subclass names itself (`who`, and `where` its tensors live), its pair limit, the text of its flat-buffer refusal, and the library's
    layout entry with the Python layout's name and slot function.  Its __init__ sets `lib`, `layout` and `count`, calls this __init__, and
    then sets `_head` (its C struct), `_sizing` (the workspace call), `_entry` (what __call__ launches) and `_extra` (that entry's
    arguments between the logits and the workspace)."""
    who = where = max_pairs = flat_text = layout_entry = layout_name = slots = None
    _entry, _extra = None, ()

    def __init__(self, shape: tuple, user_num: int, item_num: int, params, grads, device):
        """shape: the leading integers of every library call.  params and grads (None: forward only) must be contiguous fp32 [count]
        tensors on `device`, and the library must lay the parameters out as the Python layout does."""
        import torch
        for name, t in (("params", params), ("grads", grads)):
            if not (t is None and name == "grads") and (not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != device
                                                         or tuple(t.shape) != (self.count,) or not t.is_contiguous()):
                raise ValueError(self.flat_text.format(name=name, count=self.count))
        self.params, self.grads = params, grads
        self.shape, self.user_num, self.item_num = shape, int(user_num), int(item_num)
        slots = self.slots(self.layout)
        offs = (C.c_int64 * len(slots))()
        count = int(getattr(self.lib, self.layout_entry)(*self.shape, self.user_num, self.item_num, offs))
        if count != self.count or list(offs) != slots:
            raise RuntimeError(f"{self.who}: the library's parameter layout differs from {self.layout_name}")
        self._ws, self._ws_pairs = None, 0
        self.rng = self._drop = None

    def _check_rng(self, rng):
        import torch
        if (not isinstance(rng, torch.Tensor) or rng.dtype != torch.int64 or tuple(rng.shape) != (2,) or rng.device != self.params.device
                or not rng.is_contiguous()):
            raise ValueError(f"{self.who}: the dropout rng must be a contiguous int64 tensor [2] = {{seed, step}} on {self.where}")
        self.rng = rng
        return rng.data_ptr()

    def reserve(self, n: int) -> None:
        import torch
        if n <= self._ws_pairs:
            return
        nbytes = int(self._sizing(*self.shape, int(n)))
        if nbytes < 0:
            raise ValueError(f"{self.who}: n = {n} pairs outside [1, {self.max_pairs}]")
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"{self.who}: the workspace cannot grow inside a capture; call reserve(n) first")
        self._ws, self._ws_pairs = torch.empty(nbytes, dtype=torch.uint8, device=self.params.device), int(n)

    def _check(self, tensors) -> int:
        import torch
        n = int(tensors[0].shape[0])
        for t, dt in zip(tensors, (torch.int64, torch.int64, torch.float32)):
            if t.dtype != dt or tuple(t.shape) != (n,) or t.device != self.params.device or not t.is_contiguous():
                raise ValueError(f"{self.who}: users, items (int64) and labels (fp32) must be contiguous [n] tensors on {self.where}")
        self.reserve(n)
        return n

    def __call__(self, users, items, labels, loss=None, logits=None):
        import torch
        if self._entry is None:
            raise ValueError(f"{self.who}: this {type(self).__name__} was made without a gradient buffer")
        n = self._check((users, items, labels))
        dev = self.params.device
        loss = torch.empty(1, dtype=torch.float32, device=dev) if loss is None else loss
        logits = torch.empty(n, dtype=torch.float32, device=dev) if logits is None else logits
        front = (C.byref(self._head), users.data_ptr(), items.data_ptr(), labels.data_ptr(), n, loss.data_ptr(), logits.data_ptr())
        _lib.check(self._entry(*front, *self._extra, self._ws.data_ptr(), self._ws.numel(), _lib.stream()))
        return loss, logits


class PairTrainer:
    """AdamW (or, with optim="sgd", SGD) on a model of (user, item) pairs, all on the device.  The trained parameters move into ONE flat fp32
    buffer (`layout`: {state_dict key: (offset in floats, shape)}) and the model's nn.Parameters are re-pointed at views of it, so the model
    sees the trained weights with no copy.  The trainer owns the gradient buffer, exp_avg, exp_avg_sq (AdamW only), the decay mask and the
    device step counter; __init__ states the optimizer, schedule and guard options.
    max_grad_norm None or 0: no clipping.  dropout_seed=<int>: `rng` is an int64 [2] device tensor {seed, step} and `step_count` a view of
    rng[1:2]: the pmgt_op_adamw call that ends every step advances the mask stream, so eager and replayed steps draw fresh masks with no
    host write.
    A subclass sets `who`, `max_pairs` and `layouts_differ`; its __init__ validates the model, chooses the layout, calls this __init__ and
    _adopt, and builds `grad_fn`, a PairGrad over params and grads."""
    who = max_pairs = layouts_differ = None

    def __init__(self, model, dev, layout: dict, count: int, lr, weight_decay, betas, eps, max_grad_norm, dropout_seed, optim: str = "adamw",
                 scheduler_type=None, num_warmup_steps=None, num_training_steps=None, nonfinite=None, step_log: int = 0,
                 max_skipped_in_a_row: int = 25):
        """optim, scheduler_type / num_warmup_steps / num_training_steps, nonfinite, step_log, max_skipped_in_a_row: the reference's --optim,
        --scheduler-type and --mp-enabled, named and meant as pmgt_amd.trainer.Trainer states them.  What step() launches after the gradient
        entry: all defaults pmgt_op_adamw, as ever; AdamW with a schedule pmgt_op_adamw_scheduled; AdamW with nonfinite or step_log
        pmgt_op_adamw_guarded; optim="sgd" pmgt_op_sgd always (torch.optim.SGD without momentum, coupled weight decay; no moment buffers
        exist: exp_avg and exp_avg_sq are None and absent from the state).  Every decision is taken on the device, so capture / replay hold
        for every combination.  The guard logs the step's own loss; step_log() reads the ring, check_nonfinite() the counters.
        With dropout_seed the step of the mask stream is the optimizer's step counter, which counts APPLIED steps: a skipped step does not
        advance it, and the next step draws the same masks on another batch.  That is harmless and keeps a run a pure function of the seed."""
        import torch
        if optim not in ("adamw", "sgd"):
            raise ValueError(f"{self.who}: optim={optim!r}: expected 'adamw' or 'sgd'")
        if nonfinite not in (None, "skip"):
            raise ValueError(f"{self.who}: nonfinite={nonfinite!r}: expected None or 'skip'")
        if int(step_log) < 0 or int(max_skipped_in_a_row) < 1:
            raise ValueError(f"{self.who}: step_log={step_log!r} must be >= 0 and max_skipped_in_a_row={max_skipped_in_a_row!r} >= 1")
        self.optim, self.nonfinite, self.step_log_rows, self.max_skipped_in_a_row = optim, nonfinite, int(step_log), int(max_skipped_in_a_row)
        self.scheduler_type, self.num_warmup_steps, self.num_training_steps = scheduler_type, num_warmup_steps, num_training_steps
        self._sched = None
        if scheduler_type is not None:
            from .schedule import lr_lambda
            lr_lambda(scheduler_type, num_warmup_steps, num_training_steps, lr)       # refuses what the device step would refuse
            self._sched = _lib.LrScheduleC(_lib.LR_SCHEDULE_TYPES.index(scheduler_type), *self.schedule()[1:])
        self.model = model
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), (float(betas[0]), float(betas[1])), float(eps)
        self.max_grad_norm = float(max_grad_norm or 0.0)
        self.layout, self.count = layout, count
        self.params = torch.zeros(self.count, dtype=torch.float32, device=dev)
        self.grads = torch.zeros_like(self.params)
        self.exp_avg = self.exp_avg_sq = None
        if optim == "adamw":
            self.exp_avg, self.exp_avg_sq = torch.zeros_like(self.params), torch.zeros_like(self.params)
        # the guard's device state in ONE int64 buffer, so one copy reads it: counters [4], log_i [R][2], log_f [R][STEP_LOG_FLOATS] as fp32
        self._guard_state = None
        if nonfinite is not None or self.step_log_rows:
            self._guard_state = torch.zeros(4 + self.step_log_rows * (2 + _lib.STEP_LOG_FLOATS // 2), dtype=torch.int64, device=dev)
            self._reset_step_log()
        self.dropout_seed = None if dropout_seed is None else int(dropout_seed)
        if self.dropout_seed is None:
            self.rng, self.step_count = None, torch.zeros(1, dtype=torch.int64, device=dev)
        else:
            self.rng = torch.tensor([self.dropout_seed, 0], dtype=torch.int64, device=dev)
            self.step_count = self.rng[1:2]                  # the optimizer's step counter IS the step of the mask stream
        self.decay = torch.zeros(self.count, dtype=torch.uint8, device=dev)
        self._scal = torch.zeros(8, dtype=torch.float32, device=dev)
        self._part = torch.zeros(1024, dtype=torch.float32, device=dev)
        self._graph = self._static = self._logit_buf = None

    def _adopt(self, source, repoint, decays) -> None:
        """Fills the flat parameters, tensor by tensor of the layout: source(key) is copied in, the model's parameter of that name is
        re-pointed at the view where repoint(key), and the tensor's floats are marked in the decay mask where decays(key)."""
        import torch
        import torch.nn as nn
        with torch.no_grad():
            for key, (off, shape) in self.layout.items():
                view = self.params[off: off + int(np.prod(shape))].view(shape)
                view.copy_(source(key).detach())
                if repoint(key):
                    mod = self.model.get_submodule(key.rsplit(".", 1)[0])
                    setattr(mod, key.rsplit(".", 1)[1], nn.Parameter(view, requires_grad=True))
                if decays(key):
                    self.decay[off: off + int(np.prod(shape))] = 1

    def views(self, flat) -> dict:
        """{state_dict key: view of `flat`} for a buffer of the layout (params, grads, exp_avg, ...)."""
        return {k: flat[off: off + int(np.prod(shape))].view(shape) for k, (off, shape) in self.layout.items()}

    def step(self, users, items, labels, loss=None):
        """One optimizer step on the pairs (device tensors: int64 [n], int64 [n], fp32 [n]; ids inside the tables, check_pairs checks them on
        the host) -> the loss before the step as a device tensor [1].  With a seed, a TRAINING-mode step whatever model.training says.
        Five launches enqueued; no host copy, no synchronisation."""
        loss, _ = self.grad_fn(users, items, labels, loss=loss, logits=self._logits(int(users.shape[0])))
        lib = self.grad_fn.lib
        tail = (self.step_count.data_ptr(), self._scal.data_ptr(), self._part.data_ptr())
        sched, guard = self._step_options(loss)
        if self.optim == "sgd":
            _lib.check(lib.pmgt_op_sgd(self.params.data_ptr(), self.grads.data_ptr(), self.decay.data_ptr(), self.count, self.lr,
                                       self.weight_decay, self.max_grad_norm, *tail, sched, guard, _lib.stream()))
            return loss
        adam = (self.params.data_ptr(), self.grads.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(), self.decay.data_ptr(),
                self.count, self.lr, self.weight_decay, self.betas[0], self.betas[1], self.eps, self.max_grad_norm, *tail)
        if guard is not None:
            _lib.check(lib.pmgt_op_adamw_guarded(*adam, sched, guard, _lib.stream()))
        elif sched is not None:
            _lib.check(lib.pmgt_op_adamw_scheduled(*adam, sched, _lib.stream()))
        else:
            _lib.check(lib.pmgt_op_adamw(*adam, _lib.stream()))
        return loss

    def _step_options(self, loss):
        """(schedule, guard) as the optimizer entries take them, each a reference or None; the guard logs `loss`, the step's own."""
        sched = None if self._sched is None else C.byref(self._sched)
        if self._guard_state is None:
            return sched, None
        rows, base = self.step_log_rows, self._guard_state.data_ptr()
        gd = _lib.StepGuardC(base, base + 8 * (4 + 2 * rows) if rows else None, base + 8 * 4 if rows else None, rows, loss.data_ptr(),
                             1 if self.nonfinite == "skip" else 0)
        return sched, C.byref(gd)

    def schedule(self):
        """(type, W, T) of the learning-rate schedule, or None."""
        if self.scheduler_type is None:
            return None
        return (self.scheduler_type, int(self.num_warmup_steps or 0), int(self.num_training_steps or 0))

    def _reset_step_log(self) -> None:
        """Counters 0 and an empty ring (attempt -1 marks a row that holds no step)."""
        self._guard_state.zero_()
        self._guard_state[4: 4 + 2 * self.step_log_rows] = -1

    def _read_guard(self):
        """(counters dict, log_i int64 [R, 2], log_f fp32 [R, STEP_LOG_FLOATS]) from ONE device -> host copy (it waits for the steps
        launched so far)."""
        import torch
        host, rows = self._guard_state.cpu(), self.step_log_rows
        a, sk, row, _ = (int(x) for x in host[:4])
        return ({"attempts": a, "skipped": sk, "skipped_in_a_row": row}, host[4: 4 + 2 * rows].view(rows, 2),
                host[4 + 2 * rows:].view(torch.float32).view(rows, _lib.STEP_LOG_FLOATS))

    def step_counters(self):
        """{"attempts", "skipped", "skipped_in_a_row"} of the guarded step (None without a guard): one small read."""
        return None if self._guard_state is None else self._read_guard()[0]

    def step_log(self) -> list:
        """The rows of the log ring that hold a step, oldest first, as Engine.step_log() gives them: {attempt, opt_step (after the step: it
        counts applied steps), loss (the step's own), grad_norm (pre-clip), clip_coef, lr, skipped, nonfinite}.  One copy."""
        if self._guard_state is None or not self.step_log_rows:
            return []
        _, i, f = self._read_guard()
        rows = sorted((int(i[r, 0]), r) for r in range(i.shape[0]) if int(i[r, 0]) >= 0)
        return [dict(attempt=a, opt_step=int(i[r, 1]), loss=float(f[r, 0]), grad_norm=float(f[r, 1]), clip_coef=float(f[r, 2]), lr=float(f[r, 3]),
                     skipped=int(f[r, 4]) == _lib.STEP_LOG_SKIPPED, nonfinite=int(f[r, 4]) != _lib.STEP_LOG_APPLIED) for a, r in rows]

    def check_nonfinite(self):
        """Reads the step counters (one small read) and raises trainer.NonFiniteGradientsError when max_skipped_in_a_row or more optimizer
        steps in a row were skipped.  Returns the counters (None without a guard)."""
        if self._guard_state is None:
            return None
        c = self.step_counters()
        if self.nonfinite == "skip" and c["skipped_in_a_row"] >= self.max_skipped_in_a_row:
            from .trainer import NonFiniteGradientsError
            log = self.step_log()
            norm = f"{log[-1]['grad_norm']!r} (attempt {log[-1]['attempt']})" if log else "not logged (step_log=0)"
            raise NonFiniteGradientsError(
                f"{self.who}: the last {c['skipped_in_a_row']} optimizer steps in a row were skipped for a non-finite gradient norm "
                f"(max_skipped_in_a_row={self.max_skipped_in_a_row}; {c['skipped']} of {c['attempts']} steps skipped in total; last logged "
                f"pre-clip norm: {norm}); parameters and optimizer state are those of the last applied step", c)
        return c

    def _logits(self, n: int):
        import torch
        if self._logit_buf is None or self._logit_buf.numel() < n:
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"{self.who}: buffers cannot grow inside a capture")
            self._logit_buf = torch.empty(n, dtype=torch.float32, device=self.params.device)
        return self._logit_buf[:n]

    def capture(self, n: int):
        """Captures step() on `n` pairs into a graph over static input buffers -> (users, items, labels, loss): write a batch into the first
        three, replay(), read the last.  One stream.  Every buffer is created before the capture, and one warm-up step runs eagerly on the
        zeroed static batch (the kernels are loaded outside the capture) with the parameters, the moments, the step counter and the guard's
        counters and log ring put back afterwards: capturing leaves the trainer's state as it was."""
        import torch
        if not 1 <= int(n) <= self.max_pairs:
            raise ValueError(f"{self.who}: n = {n} pairs outside [1, {self.max_pairs}]")
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
            raise RuntimeError(f"{self.who}: capture(n) comes before replay()")
        self._graph.replay()
        return self._static[3]

    def state_dict(self) -> dict:
        """The flat parameters, both moments (AdamW), the step counter and the layout (which names every tensor inside the parameters, a
        trained item table among them, so a state saved for another shape or setting is refused); with dropout, the seed (with "step", the
        whole state of the mask stream); "optim" and "schedule" (the triple (type, W, T) or None); with a guard, its counters and log ring."""
        sd = {"params": self.params.detach().clone(), "step": self.step_count.clone(),
              "layout": {k: (off, tuple(shape)) for k, (off, shape) in self.layout.items()}, "optim": self.optim, "schedule": self.schedule()}
        if self.optim == "adamw":                            # (an SGD trainer holds no moments: neither key)
            sd["exp_avg"], sd["exp_avg_sq"] = self.exp_avg.clone(), self.exp_avg_sq.clone()
        if self.dropout_seed is not None:
            sd["dropout_seed"] = self.dropout_seed
        if self._guard_state is not None:                    # the guard's counters, and the log ring (log_i rows, then log_f rows as int64 words)
            sd["step_counters"], sd["step_log"] = self._guard_state[:4].clone(), self._guard_state[4:].clone()
        return sd

    def load_state_dict(self, sd: dict) -> None:
        """A state of another layout, dropout seed, optimizer or schedule is refused before anything is written.  A state from before the
        options existed (no "optim", no "schedule") is AdamW at a constant rate.  Without counters in the state a guarded trainer's start at
        0; a ring of another size is emptied."""
        import torch
        if {k: (off, tuple(shape)) for k, (off, shape) in self.layout.items()} != dict(sd["layout"]):
            raise ValueError(f"{self.who}: {self.layouts_differ}")
        if sd.get("dropout_seed") != self.dropout_seed:
            raise ValueError(f"{self.who}: the state was saved with dropout_seed = {sd.get('dropout_seed')!r}, this trainer has "
                             f"{self.dropout_seed!r}")
        if sd.get("optim", "adamw") != self.optim:
            raise ValueError(f"{self.who}: the state was saved with optim = {sd.get('optim', 'adamw')!r}, this trainer has {self.optim!r}")
        theirs = None if sd.get("schedule") is None else tuple(sd["schedule"])
        if theirs != self.schedule():
            raise ValueError(f"{self.who}: the state was saved with schedule = {theirs!r}, this trainer has {self.schedule()!r}")
        with torch.no_grad():
            self.params.copy_(sd["params"])
            if self.optim == "adamw":
                self.exp_avg.copy_(sd["exp_avg"])
                self.exp_avg_sq.copy_(sd["exp_avg_sq"])
            self.step_count.copy_(sd["step"])
            if self._guard_state is not None:
                self._reset_step_log()
                if sd.get("step_counters") is not None:
                    self._guard_state[:4].copy_(sd["step_counters"])
                    if sd["step_log"].numel() == self._guard_state.numel() - 4:
                        self._guard_state[4:].copy_(sd["step_log"])


LAST_FORMAT = "pmgt_amd.fit_pairs"      # the "format" entry of a last.ckpt fit_pairs wrote


# ---- what the epoch loops that write last.ckpt share (fit_pairs here, fit_pmgt_ncf of finetune.py) ---------------------------------------------
def run_record(trainer, batch_size: int, num_ng: int, seed: int, early_criterion: str, patience: int, max_epochs: int) -> dict:
    """The settings of a fit call that a resumed run must repeat: they fix the epoch order, the sampled pairs and the callbacks; with a
    schedule, max_epochs too (it sets the schedule's length)."""
    run = {"batch_size": int(batch_size), "num_ng": int(num_ng), "seed": int(seed), "early_criterion": early_criterion, "patience": int(patience)}
    if trainer.schedule() is not None:
        run["max_epochs"] = int(max_epochs)
    return run


def check_run_record(who: str, recorded: dict, run: dict) -> None:
    """ValueError in the name of `who`, both values named, for the first setting of `run` that the checkpoint recorded differently."""
    for k, v in run.items():
        if recorded.get(k) != v:
            raise ValueError(f"{who}(resume_from=...): the checkpoint was written with {k} = {recorded.get(k)!r}, this call has {v!r}: "
                             "the epoch order, the sampled pairs and the schedule would not continue it")


def load_last(who: str, path: str, dev, fmt: str) -> dict:
    """The last.ckpt at `path` as plain data (torch.load(weights_only=True): tensors, dicts, lists, tuples, numbers, strings; no code is
    unpickled); ValueError in the name of `who` for a file whose "format" is not `fmt`."""
    import pickle
    import torch
    try:
        ck = torch.load(path, map_location=dev, weights_only=True)
    except pickle.UnpicklingError:
        ck = None
    if not isinstance(ck, dict) or ck.get("format") != fmt:
        raise ValueError(f"{who}(resume_from=...): the checkpoint was not written by {who} (no epoch position in it)")
    return ck


def save_atomic(obj, path: str) -> None:
    """torch.save to a temporary name beside `path`, then os.replace: a reader never sees half a file."""
    import torch
    tmp = path + ".tmp"
    torch.save(obj, tmp)
    os.replace(tmp, path)


def fit_pairs(trainer, pairs, batch_size: int, max_epochs: int, num_ng: int, seed: int, early_criterion: str, patience: int, ckpt_dir: str,
              validate, checkpoint, log=None, save_last: bool = False, resume_from=None) -> list:
    """The epoch loop of fit_ncf and fit_dcn over `trainer` (a PairTrainer) and the checked interaction list `pairs` int64 [P, 2]: every epoch
    draws ng_sample(seed + epoch) and visits it in the order fit_loop.epoch_order(seed, epoch); the epoch's users, items and labels are
    uploaded once and the steps run on slices (the last batch may be short), their losses stay on the device and are read once per epoch,
    after validate(epoch) -> {metric: value} (the epoch's one wait; the model is in eval mode throughout).  early_criterion names the
    metric EarlyStopping / BestCheckpoint of fit_loop.py watch.  The best epoch's parameters are kept on the device and restored at the
    end; with ckpt_dir, checkpoint(epoch, row) -> the dict saved as the best file, the previous best file removed.
    The optimizer, the schedule and the guard are the trainer's (PairTrainer's options); with nonfinite="skip" check_nonfinite() runs once
    an epoch, after validate -- the epoch's existing wait.
    save_last=True (needs ckpt_dir): after every epoch, and BEFORE log(row), ckpt_dir/last.ckpt is written (to a temporary name, then
    os.replace): trainer.state_dict(), the epoch, the EarlyStopping and BestCheckpoint state, the best parameters and the best file's path,
    the history, and the call's batch_size, num_ng, seed, early_criterion, patience (with a schedule, max_epochs too: it sets the
    schedule's length).  So that the file can say whether the run has stopped, EarlyStopping is updated BEFORE log(row) in every run (it
    used to be after; log never sees its state, and the break still follows log, so nothing a caller can observe moves).  The file is plain
    data and is read with torch.load(weights_only=True): no code is unpickled.  resume_from=<path> or "last" restores all of it and continues at the next epoch; a recorded setting that differs
    from the call's, and a file fit_pairs did not write, are refused.  ng_sample(seed + epoch) and epoch_order(seed, epoch) are pure
    functions of the epoch and every kernel gives the same bits for the same inputs, so the resumed run is the uninterrupted one bit for bit.
    -> the history, one dict per epoch: epoch, train_loss (mean over the steps), the metrics, best (whether it improved)."""
    import torch
    from .fit_loop import BestCheckpoint, EarlyStopping, epoch_order, monitor_of
    model, dev = trainer.model, trainer.params.device
    monitor, mode = monitor_of(early_criterion)
    stopper = EarlyStopping(monitor, patience, mode)
    keeper = BestCheckpoint(ckpt_dir or "", monitor, mode)
    if (save_last or resume_from == "last") and not ckpt_dir:
        raise ValueError("fit_pairs: save_last=True and resume_from='last' need ckpt_dir")
    if ckpt_dir:
        os.makedirs(ckpt_dir, exist_ok=True)
    last_path = os.path.join(ckpt_dir, "last.ckpt") if ckpt_dir else None
    run = run_record(trainer, batch_size, num_ng, seed, early_criterion, patience, max_epochs)
    best_params, history, first_epoch, stopped = None, [], 0, False
    if resume_from is not None:
        ck = load_last("fit_pairs", last_path if resume_from == "last" else resume_from, dev, LAST_FORMAT)
        check_run_record("fit_pairs", ck["run"], run)
        trainer.load_state_dict(ck["trainer"])
        stopper.load_state_dict(ck["early_stopping"])
        keeper.load_state_dict(ck["best_checkpoint"])
        best_params, history = ck["best_params"], [dict(h) for h in ck["history"]]
        first_epoch, stopped = int(ck["epoch"]) + 1, bool(ck["stopped"])
    was_training = model.training
    model.eval()
    try:
        for epoch in range(first_epoch, 0 if stopped else int(max_epochs)):
            users, items, labels = ng_sample(pairs, model.user_num, model.item_num, num_ng, seed + epoch)
            order = epoch_order(len(users), seed, epoch)
            users_d, items_d, labels_d = (torch.from_numpy(np.ascontiguousarray(a[order])).to(dev) for a in (users, items, labels))
            n_steps = (len(order) + batch_size - 1) // batch_size
            losses = torch.empty(n_steps, 1, dtype=torch.float32, device=dev)
            for s in range(n_steps):
                lo, hi = s * batch_size, min((s + 1) * batch_size, len(order))
                trainer.step(users_d[lo:hi], items_d[lo:hi], labels_d[lo:hi], loss=losses[s])
            metrics = validate(epoch)
            if trainer.nonfinite == "skip":
                trainer.check_nonfinite()                    # (after the epoch's one wait: the read adds none)
            row = {"epoch": epoch, "train_loss": float(losses.double().mean().item()), **metrics}
            write, remove = keeper.update(epoch, row[early_criterion])
            row["best"] = write is not None
            if write is not None:
                best_params = trainer.params.detach().clone()
                if ckpt_dir:
                    torch.save(checkpoint(epoch, row), write)
                    if remove and os.path.exists(remove):
                        os.remove(remove)
            history.append(row)
            stopped = stopper.update(row[early_criterion], epoch)
            if save_last:
                save_atomic({"format": LAST_FORMAT, "trainer": trainer.state_dict(), "epoch": epoch, "early_stopping": stopper.state_dict(),
                             "best_checkpoint": keeper.state_dict(), "best_params": best_params, "history": history, "run": run,
                             "stopped": stopped}, last_path)
            if log is not None:
                log(row)
            if stopped:
                break
        if best_params is not None:
            with torch.no_grad():
                trainer.params.copy_(best_params)
    finally:
        model.train(was_training)
    return history
