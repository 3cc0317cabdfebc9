"""How a model is trained on (user, item, label) pairs on the device, stated once for the two pair heads -- the NCF head (ncf_head.py,
ncf_train.py) and the Deep & Cross Network (dcn_head.py, dcn_train.py):

  host side, numpy   ng_sample, normalize_item_table, check_ids, check_pairs, head_weights, bce_with_logits_host, and the one RNG of every
                     kernel: check_dropout_p, dropout_keep, dropout_scale, per_layer, check_seed
  PairGrad           a gradient entry over one flat parameter buffer: the buffer and layout checks, the workspace, the checked inputs
  PairTrainer        the flat buffers of AdamW, the {seed, step} tensor, step() = the gradient entry + pmgt_op_adamw, capture / replay, the state
  fit_pairs          the epoch loop: sampled pairs, steps on slices, validation, early stopping, the best parameters kept and restored

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
    """AdamW on a model of (user, item) pairs, all on the device.  The trained parameters move into ONE flat fp32 buffer (`layout`:
    {state_dict key: (offset in floats, shape)}) and the model's nn.Parameters are re-pointed at views of it, so the model sees the trained
    weights with no copy.  The trainer owns the gradient buffer, exp_avg, exp_avg_sq, the decay mask and the device step counter.
    max_grad_norm None or 0: no clipping.  dropout_seed=<int>: `rng` is an int64 [2] device tensor {seed, step} and `step_count` a view of
    rng[1:2]: the pmgt_op_adamw call that ends every step advances the mask stream, so eager and replayed steps draw fresh masks with no
    host write.
    A subclass sets `who`, `max_pairs` and `layouts_differ`; its __init__ validates the model, chooses the layout, calls this __init__ and
    _adopt, and builds `grad_fn`, a PairGrad over params and grads."""
    who = max_pairs = layouts_differ = None

    def __init__(self, model, dev, layout: dict, count: int, lr, weight_decay, betas, eps, max_grad_norm, dropout_seed):
        import torch
        self.model = model
        self.lr, self.weight_decay, self.betas, self.eps = float(lr), float(weight_decay), (float(betas[0]), float(betas[1])), float(eps)
        self.max_grad_norm = float(max_grad_norm or 0.0)
        self.layout, self.count = layout, count
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
        _lib.check(self.grad_fn.lib.pmgt_op_adamw(self.params.data_ptr(), self.grads.data_ptr(), self.exp_avg.data_ptr(),
                                                  self.exp_avg_sq.data_ptr(), self.decay.data_ptr(), self.count, self.lr, self.weight_decay,
                                                  self.betas[0], self.betas[1], self.eps, self.max_grad_norm, self.step_count.data_ptr(),
                                                  self._scal.data_ptr(), self._part.data_ptr(), _lib.stream()))
        return loss

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
        zeroed static batch (the kernels are loaded outside the capture) with the parameters, the moments and the step counter put back
        afterwards: capturing leaves the trainer's state as it was."""
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
        """The flat parameters, both moments, the step counter and the layout (which names every tensor inside the parameters, a trained
        item table among them, so a state saved for another shape or setting is refused); with dropout, the seed (with "step", the whole
        state of the mask stream)."""
        sd = {"params": self.params.detach().clone(), "exp_avg": self.exp_avg.clone(), "exp_avg_sq": self.exp_avg_sq.clone(),
              "step": self.step_count.clone(), "layout": {k: (off, tuple(shape)) for k, (off, shape) in self.layout.items()}}
        if self.dropout_seed is not None:
            sd["dropout_seed"] = self.dropout_seed
        return sd

    def load_state_dict(self, sd: dict) -> None:
        import torch
        if {k: (off, tuple(shape)) for k, (off, shape) in self.layout.items()} != dict(sd["layout"]):
            raise ValueError(f"{self.who}: {self.layouts_differ}")
        if sd.get("dropout_seed") != self.dropout_seed:
            raise ValueError(f"{self.who}: the state was saved with dropout_seed = {sd.get('dropout_seed')!r}, this trainer has "
                             f"{self.dropout_seed!r}")
        with torch.no_grad():
            self.params.copy_(sd["params"])
            self.exp_avg.copy_(sd["exp_avg"])
            self.exp_avg_sq.copy_(sd["exp_avg_sq"])
            self.step_count.copy_(sd["step"])


def fit_pairs(trainer, pairs, batch_size: int, max_epochs: int, num_ng: int, seed: int, early_criterion: str, patience: int, ckpt_dir: str,
              validate, checkpoint, log=None) -> list:
    """The epoch loop of fit_ncf and fit_dcn over `trainer` (a PairTrainer) and the checked interaction list `pairs` int64 [P, 2]: every epoch
    draws ng_sample(seed + epoch) and visits it in the order fit_loop.epoch_order(seed, epoch); the epoch's users, items and labels are
    uploaded once and the steps run on slices (the last batch may be short), their losses stay on the device and are read once per epoch,
    after validate(epoch) -> {metric: value} (the epoch's one wait; the model is in eval mode throughout).  early_criterion names the
    metric EarlyStopping / BestCheckpoint of fit_loop.py watch.  The best epoch's parameters are kept on the device and restored at the
    end; with ckpt_dir, checkpoint(epoch, row) -> the dict saved as the best file, the previous best file removed.
    -> the history, one dict per epoch: epoch, train_loss (mean over the steps), the metrics, best (whether it improved)."""
    import torch
    from .fit_loop import BestCheckpoint, EarlyStopping, epoch_order, monitor_of
    model, dev = trainer.model, trainer.params.device
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
            metrics = validate(epoch)
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
            if log is not None:
                log(row)
            if stopper.update(row[early_criterion], epoch):
                break
        if best_params is not None:
            with torch.no_grad():
                trainer.params.copy_(best_params)
    finally:
        model.train(was_training)
    return history
