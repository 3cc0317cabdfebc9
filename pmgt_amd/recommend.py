"""Recommendation from the whole catalogue: for a batch of users, the k best items of a trained PMGT_NCF that the user has not interacted
with.  The reference has no such path (its test step, pmgt/ncf/trainer.py:202-219, does `pred.topk(100)` on one sampled candidate list per
user); here the head (pmgt/pmgt_ncf/models.py:91-105) is fused into one HIP kernel that scores every (user, item) pair of a batch without
materialising pair rows (pmgt_ncf_score), and a second kernel selects per row (pmgt_topk_rows).

THE ORDER is that of the ranking metrics: descending `score_key`, and among equal keys THE LOWER ITEM INDEX FIRST.

The pure-numpy part (topk_host, exclusion_csr) needs no GPU; the head (its shape, the covered heads, ncf_head_host) is stated in ncf_head.py."""
import contextlib
import ctypes as C

import numpy as np

from . import _lib
from ._lib import NCF_FACTORS, NCF_MAX_D, NCF_MAX_LAYERS, NCF_MAX_USERS, TOPK_FLAG_NAN, TOPK_FLAG_SHORT, TOPK_MAX_K  # noqa: F401
from .evaluation import score_key
from .ncf_model import check_ncf_model_covered
from .ncf_head import check_head_covered, check_ids, check_item_table, head_shape, head_state, ncf_head_host  # noqa: F401
from .dcn_head import ITEM_KEY, USER_KEY, check_dcn_covered, dcn_layout, dcn_scores_host, dcn_shape  # noqa: F401

SCORE_WORKSPACE_BYTES = 256 << 20                # recommend(batch_users=None): the [batch, I] fp32 score rows stay within this


# ---- host side: pure numpy ------------------------------------------------------------------------------------------------------------------
def check_k(k) -> int:
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or not 1 <= int(k) <= TOPK_MAX_K:
        raise ValueError(f"k = {k!r}: expected an integer in [1, {TOPK_MAX_K}]")
    return int(k)


def check_csr(indptr, items, user_num: int, item_num: int, who: str = "exclude", what: str = "excluded items"):
    """(indptr int64 [user_num + 1], items int32) validated as pmgt_topk_rows expects its CSR: indptr non-decreasing from 0 to len(items), items in
    [0, item_num).  `who` and `what` name the list in the messages (the exclusion list unless told otherwise)."""
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    items64 = np.ascontiguousarray(items, dtype=np.int64)
    if indptr.shape != (user_num + 1,) or items64.ndim != 1:
        raise ValueError(f"{who}: indptr {indptr.shape} must be [user_num + 1 = {user_num + 1}] and items one-dimensional")
    if indptr[0] != 0 or indptr[-1] != len(items64) or (np.diff(indptr) < 0).any():
        raise ValueError(f"{who}: indptr must be non-decreasing from 0 to len(items)")
    check_ids(what, items64, item_num, who)
    return indptr, items64.astype(np.int32)


def exclusion_csr(exclude, user_num: int, item_num: int, who: str = "exclude", what: str = "excluded items"):
    """The exclusion CSR over user ids from `exclude`: None (nothing excluded), an iterable of (user, item) pairs -- typically the training
    interactions --, or a ready (indptr, items) pair of arrays.  -> (indptr int64 [user_num + 1], items int32), each list sorted by item.
    `who` and `what` name the list in the messages: another list of pairs over the same ids (the held-out set) is built the same way."""
    if isinstance(exclude, tuple) and len(exclude) == 2 and all(isinstance(a, np.ndarray) and a.ndim == 1 for a in exclude) \
            and len(exclude[0]) == user_num + 1:
        return check_csr(exclude[0], exclude[1], user_num, item_num, who, what)
    pairs = np.asarray(exclude if isinstance(exclude, np.ndarray) else list(exclude or ()))
    if pairs.size == 0:
        return np.zeros(user_num + 1, dtype=np.int64), np.zeros(0, dtype=np.int32)
    if pairs.ndim != 2 or pairs.shape[1] != 2 or not np.issubdtype(pairs.dtype, np.integer):
        raise ValueError(f"{who}: expected (user, item) integer pairs, got an array of shape {pairs.shape} and dtype {pairs.dtype}")
    pairs = pairs.astype(np.int64)
    check_ids("users", pairs[:, 0], user_num, who)
    check_ids(what, pairs[:, 1], item_num, who)
    order = np.lexsort((pairs[:, 1], pairs[:, 0]))
    indptr = np.zeros(user_num + 1, dtype=np.int64)
    np.cumsum(np.bincount(pairs[:, 0], minlength=user_num), out=indptr[1:])
    return indptr, pairs[order, 1].astype(np.int32)


def topk_host(scores, k: int, indptr=None, items=None, users=None):
    """The yardstick of pmgt_topk_rows, pure numpy: per row of scores [n, I] the k best eligible items by a STABLE argsort on descending
    `score_key` (NaN first, -0.0 and 0.0 tie; among equal keys the lower item index first).  Item j is excluded for row r iff it is in the
    list indptr[users[r]] .. indptr[users[r] + 1] of `items` (indptr None: everything is eligible).
    -> (items int32 [n, k], scores fp32 [n, k], flags uint32 [n]): -1 / -inf past the eligible count; flag bit 0 = a NaN among the eligible
    scores, bit 1 = fewer than k eligible items."""
    k = check_k(k)
    x = np.ascontiguousarray(scores, dtype=np.float32)
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError(f"topk_host: scores {x.shape} must be [n, I] with I >= 1")
    n, n_items = x.shape
    eligible = np.ones((n, n_items), dtype=bool)
    if indptr is not None:
        users = np.asarray(users, dtype=np.int64)
        for r in range(n):
            eligible[r, np.asarray(items[indptr[users[r]]: indptr[users[r] + 1]], dtype=np.int64)] = False
    # descending by key, stable: ascending in (2^32 - 1 - key); the excluded behind every eligible item
    inv = np.where(eligible, np.int64(0xFFFFFFFF) - score_key(x).reshape(n, n_items).astype(np.int64), np.int64(1) << 32)
    order = np.argsort(inv, axis=1, kind="stable")
    count = eligible.sum(axis=1)
    out_items = np.full((n, k), -1, dtype=np.int32)
    out_scores = np.full((n, k), -np.inf, dtype=np.float32)
    kk = min(k, n_items)
    live = np.arange(kk)[None, :] < count[:, None]
    out_items[:, :kk] = np.where(live, order[:, :kk], -1)
    out_scores[:, :kk] = np.where(live, np.take_along_axis(x, order[:, :kk], axis=1), np.float32(-np.inf))
    flags = ((np.isnan(x) & eligible).any(axis=1) * TOPK_FLAG_NAN + (count < k) * TOPK_FLAG_SHORT).astype(np.uint32)
    return out_items, out_scores, flags


# ---- the checks the whole-catalogue drivers share (recommend, evaluate_catalogue, similar_items, evaluate_neighbours) -------------------------
def check_impl(impl) -> str:
    if impl not in ("host", "device"):
        raise ValueError(f"impl={impl!r}: expected 'host' or 'device'")
    return impl


def check_batch(batch, n_ids: int, n_items: int, who: str, name: str = "batch_users") -> int:
    """The ids per launch from the caller's `batch_users` / `batch_items` (`name`): None picks default_batch_users."""
    if batch is not None and (not isinstance(batch, (int, np.integer)) or isinstance(batch, bool) or batch < 1):
        raise ValueError(f"{who}: {name} = {batch!r} must be a positive integer or None")
    return default_batch_users(n_ids, n_items) if batch is None else int(min(batch, n_ids, NCF_MAX_USERS))


def refuse_nan(who: str, n_nan: int, n_ids: int, what: str) -> None:
    """`what`: "users" or "items", the ids that were scored."""
    if n_nan:
        raise ValueError(f"{who}: {n_nan} of {n_ids} {what} have a NaN score among their eligible items")


# ---- device side ------------------------------------------------------------------------------------------------------------------------------
class CatalogueScorer:
    """What select_device and catalogue_eval.rank_device need of a scorer: `device`, `n_items` (set by the subclass's constructor) and
    score(ids, out=None): ids int64 [n] on the device (the caller checks their range on the host) -> scores fp32 [n, row_stride] with the
    score of (ids[r], item j) at [r, j]; `out` (fp32, contiguous, [>= n, row_stride >= I]) is written in place and entries [r, I ..) are
    left.  A subclass names its entry (`entry`, the prefix of the messages) and its ids (`ids_name`) and launches in
    _launch(ids, n, out).  `max_ids`: the upper bound on n that is refused here; None leaves it to the entry (RuntimeError)."""
    entry = None
    ids_name = "users"
    place = "the table's device"
    max_ids = None

    def score(self, ids, out=None):
        import torch
        n = int(ids.shape[0])
        if ids.dtype != torch.int64 or ids.dim() != 1 or ids.device != self.device or not ids.is_contiguous() or n < 1 \
                or (self.max_ids is not None and n > self.max_ids):
            span = "n >= 1" if self.max_ids is None else f"1 .. {self.max_ids}"
            raise ValueError(f"{self.entry}: {self.ids_name} must be a contiguous int64 tensor [{span}] on {self.place}")
        if out is None:
            out = torch.empty(n, self.n_items, dtype=torch.float32, device=self.device)
        if out.dtype != torch.float32 or out.dim() != 2 or not out.is_contiguous() or out.shape[0] < n or out.shape[1] < self.n_items \
                or out.device != self.device:
            raise ValueError(f"{self.entry}: out must be a contiguous fp32 tensor [>= {n}, >= {self.n_items}] on {self.place}")
        self._launch(ids, n, out)
        return out


class NcfScorer(CatalogueScorer):
    """The fused head over one item table: NcfScorer(weights, table) splits layer 0 and computes the per-item half Pi = table W0e^T + b0
    once; score(users) computes the per-user half Pu = U_mlp[users] W0u^T (a torch matmul: plumbing) and launches pmgt_ncf_score.
    `weights`: the head's parameters as contiguous fp32 DEVICE tensors keyed like the state_dict (a PMGT_NCF's own state_dict serves);
    `table` [I, d] fp32 on the same device.  Nothing in here copies to the host or waits for the device."""
    entry = "ncf_score"

    def __init__(self, weights: dict, table):
        import torch
        self.lib = _lib.hip()
        self.factor, self.num_layers, self.kind, self.d = head_shape(weights)
        check_head_covered(self.factor, self.num_layers, self.kind)
        need = ["mlp_user_embeddings.weight", "predict_layer.weight", "predict_layer.bias"]
        need += [f"mlp_layers.{i}.linear.{p}" for i in range(self.num_layers) for p in ("weight", "bias")]
        need += ["gmf_user_embeddings.weight", "gmf_item_embeddings.weight"] if self.kind == "NeuMF-end" else []
        check_item_table(table, None, self.d, None, "ncf_score")
        self.w = {}
        for key in need:
            t = weights[key]
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != table.device:
                raise ValueError(f"ncf_score: {key} must be an fp32 tensor on the table's device")
            self.w[key] = t.detach().contiguous()
        self.device, self.n_items = table.device, int(table.shape[0])
        self.user_num = int(self.w["mlp_user_embeddings.weight"].shape[0])
        w0 = self.w["mlp_layers.0.linear.weight"]
        if tuple(w0.shape) != (self.d, 2 * self.d):
            raise ValueError(f"ncf_score: mlp_layers.0.linear.weight {tuple(w0.shape)} must be [{self.d}, {2 * self.d}]")
        if self.kind == "NeuMF-end" and self.w["gmf_item_embeddings.weight"].shape[0] < self.n_items:
            raise ValueError("ncf_score: gmf_item_embeddings.weight has fewer rows than the item table")
        self._w0u_t = w0[:, :self.d].t().contiguous()
        self.pi = torch.addmm(self.w["mlp_layers.0.linear.bias"], table, w0[:, self.d:].t()).contiguous()
        h = _lib.NcfHeadC()
        h.factor_num, h.num_layers, h.kind, h.user_num = self.factor, self.num_layers, _lib.NCF_KINDS.index(self.kind), self.user_num
        for i in range(1, self.num_layers):
            h.weight[i] = self.w[f"mlp_layers.{i}.linear.weight"].data_ptr()
            h.bias[i] = self.w[f"mlp_layers.{i}.linear.bias"].data_ptr()
        h.predict_weight, h.predict_bias = self.w["predict_layer.weight"].data_ptr(), self.w["predict_layer.bias"].data_ptr()
        if self.kind == "NeuMF-end":
            h.gmf_user, h.gmf_item = self.w["gmf_user_embeddings.weight"].data_ptr(), self.w["gmf_item_embeddings.weight"].data_ptr()
        self._head = h

    def _launch(self, users, n, out):
        pu = self.w["mlp_user_embeddings.weight"].index_select(0, users) @ self._w0u_t
        _lib.check(self.lib.pmgt_ncf_score(C.byref(self._head), pu.data_ptr(), self.pi.data_ptr(), users.data_ptr(), n, self.n_items,
                                           out.data_ptr(), int(out.shape[1]), _lib.stream()))


class NcfModelScorer(CatalogueScorer):
    """NcfScorer for the reference's stand-alone NCF class (ncf.py): the fused eval-mode head with or without LayerNorm, kinds MLP, GMF,
    NeuMF-end and NeuMF-pre (scored as NeuMF-end), by pmgt_ncf_model_score.  `weights`: the model's parameters as fp32 DEVICE tensors keyed
    like its state_dict (a whole state_dict serves: pass kind=, which a state_dict alone does not tell); `table` [I, d] fp32 on the same
    device stands in for embed_item_MLP.weight (None: that tensor).  Pi = table W0e^T + b0 is computed once; score(users) computes Pu and
    launches.  Kind GMF has no Pi / Pu and refuses a `table`.  Nothing in here copies to the host or waits for the device."""
    entry = "ncf_model_score"

    def __init__(self, weights: dict, table=None, kind: str = None, layer_norm_eps: float = 1e-12):
        import torch
        from . import ncf_model as M
        self.lib = _lib.hip()
        self.factor, self.num_layers, self.kind, self.ln = M.ncf_model_shape(weights, kind)
        mlp, gmf = M.reads_mlp(self.kind), M.reads_gmf(self.kind)
        M.check_ncf_model_covered(self.factor, self.num_layers if mlp else 1, self.kind, layer_norm_eps)      # (GMF: whatever layers the weights hold)
        self.d = self.factor << (self.num_layers - 1) if mlp else 0
        need = [M.OUT_W, M.OUT_B] + ([M.USER_GMF, M.ITEM_GMF] if gmf else [])
        if mlp:
            need += [M.USER_MLP] + [k for i in range(self.num_layers) for k in M.layer_keys(i, self.ln)]
            if table is None:
                table = weights[M.ITEM_MLP].detach()
            check_item_table(table, None, self.d, None, "ncf_model_score")
            device = table.device
        else:
            if table is not None:
                raise ValueError("ncf_model_score: kind 'GMF' reads no item table")
            device = weights[M.ITEM_GMF].device
            if device.type != "cuda":
                raise ValueError("ncf_model_score: the weights must be on a GPU")
        self.w = {}
        for key in need:
            t = weights[key]
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != device:
                raise ValueError(f"ncf_model_score: {key} must be an fp32 tensor on the table's device")
            self.w[key] = t.detach().contiguous()
        self.device = device
        self.n_items = int(table.shape[0] if mlp else self.w[M.ITEM_GMF].shape[0])
        self.user_num = int(self.w[M.USER_MLP if mlp else M.USER_GMF].shape[0])
        if tuple(self.w[M.OUT_W].shape) != (1, self.factor * (2 if mlp and gmf else 1)):
            raise ValueError(f"ncf_model_score: predict_layer.weight {tuple(self.w[M.OUT_W].shape)} does not fit kind {self.kind!r}")
        if gmf and (self.w[M.ITEM_GMF].shape[0] < self.n_items or self.w[M.USER_GMF].shape[0] != self.user_num
                    or self.w[M.ITEM_GMF].shape[1] != self.factor):
            raise ValueError("ncf_model_score: the GMF tables do not fit the MLP tables")
        h = _lib.NcfModelHeadC()
        h.factor_num, h.num_layers, h.kind, h.user_num = self.factor, max(self.num_layers, 1), _lib.NCF_MODEL_KINDS.index(self.kind), self.user_num
        h.use_layer_norm, h.layer_norm_eps = int(self.ln), float(layer_norm_eps)
        self.pi = self._w0u_t = None
        if mlp:
            for i in range(self.num_layers):
                keys = M.layer_keys(i, self.ln)
                out = self.d >> i
                if tuple(self.w[keys[0]].shape) != (out, 2 * out) or any(tuple(self.w[k].shape) != (out,) for k in keys[1:]):
                    raise ValueError(f"ncf_model_score: the tensors of layer {i} must be [{out}, {2 * out}] and [{out}]")
                if i:
                    h.weight[i], h.bias[i] = self.w[keys[0]].data_ptr(), self.w[keys[1]].data_ptr()
                if self.ln:
                    h.gamma[i], h.beta[i] = self.w[keys[2]].data_ptr(), self.w[keys[3]].data_ptr()
            w0, b0 = (self.w[k] for k in M.layer_keys(0, self.ln)[:2])
            self._w0u_t = w0[:, :self.d].t().contiguous()
            self.pi = torch.addmm(b0, table, w0[:, self.d:].t()).contiguous()
        h.predict_weight, h.predict_bias = self.w[M.OUT_W].data_ptr(), self.w[M.OUT_B].data_ptr()
        if gmf:
            h.gmf_user, h.gmf_item = self.w[M.USER_GMF].data_ptr(), self.w[M.ITEM_GMF].data_ptr()
        self._user_mlp = self.w[M.USER_MLP] if mlp else None
        self._head = h

    def _launch(self, users, n, out):
        pu = self._user_mlp.index_select(0, users) @ self._w0u_t if self.pi is not None else None
        _lib.check(self.lib.pmgt_ncf_model_score(C.byref(self._head), pu.data_ptr() if pu is not None else 0,
                                                 self.pi.data_ptr() if pu is not None else 0, users.data_ptr(), n, self.n_items,
                                                 out.data_ptr(), int(out.shape[1]), _lib.stream()))


class DcnScorer(CatalogueScorer):
    """NcfModelScorer for the Deep & Cross Network (dcn.py): the fused eval-mode model by pmgt_dcn_score, the deep tower on the NCF scoring
    tile and the collapsed cross net (dcn_head.py's header) in its epilogue.  `weights_or_flat`: the model's parameters as fp32 DEVICE
    tensors keyed like its state_dict (a whole state_dict serves; they are gathered into one flat buffer of dcn_layout once), or a pair
    (dims, flat) = ((factor_num, deep_layers, cross_layers, use_layer_norm, user_num, item_num), the flat fp32 parameter buffer of that
    layout) -- a DcnTrainer's `params` is then READ IN PLACE, no copy.  `table` [I, E] fp32 on the same device stands in for
    item_embeddings.weight (None: that tensor).  Built once: Pi = table W0i^T + b0, the item rows' scalars (pmgt_dcn_score_rows) and the 2 C
    constants K_c, B_c (torch: plumbing); they are a snapshot of the parameters at construction.  score(users) gathers the user rows,
    computes Pu and their scalars and launches.  Nothing in here copies to the host or waits for the device."""
    entry, place = "dcn_score", "the parameters' device"

    def __init__(self, weights_or_flat, table=None, layer_norm_eps: float = 1e-12):
        import torch
        if isinstance(weights_or_flat, dict):
            w = weights_or_flat
            factor, deep, cross, ln = dcn_shape(w)
            check_dcn_covered(factor, deep, cross)
            dims = (factor, deep, cross, ln, int(w[USER_KEY].shape[0]), int(w[ITEM_KEY].shape[0]))
            layout, count = dcn_layout(*dims)
            device = w[USER_KEY].device
            for key, (_, shape) in layout.items():
                t = w[key]
                if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != device or tuple(t.shape) != tuple(shape):
                    raise ValueError(f"dcn_score: {key} must be an fp32 tensor {tuple(shape)} on the user table's device")
            flat = torch.empty(count, dtype=torch.float32, device=device)
            for key, (off, shape) in layout.items():
                flat[off: off + int(np.prod(shape))].view(shape).copy_(w[key].detach())
        else:
            dims, flat = weights_or_flat
            dims = tuple(int(v) for v in dims)
            check_dcn_covered(*dims[:3])
            layout, count = dcn_layout(*dims[:3], bool(dims[3]), *dims[4:])
            if not isinstance(flat, torch.Tensor) or flat.dtype != torch.float32 or tuple(flat.shape) != (count,) or not flat.is_contiguous():
                raise ValueError(f"dcn_score: the flat parameters must be a contiguous fp32 tensor [{count}]")
            flat = flat.detach()
        eps = float(np.float32(layer_norm_eps))
        if not (np.isfinite(eps) and eps >= 0.0):
            raise ValueError(f"dcn_score: layer_norm_eps = {layer_norm_eps!r} is not finite or negative")
        if flat.device.type != "cuda":
            raise ValueError("dcn_score: the parameters must be on a GPU")
        self.lib = _lib.hip()
        self.factor, self.deep, self.cross, self.ln, self.user_num, _ = dims
        self.ln = bool(self.ln)
        self.d = E = self.factor << self.deep
        self.device, self.flat = flat.device, flat

        def view(key):
            off, shape = layout[key]
            return flat[off: off + int(np.prod(shape))].view(shape)
        if table is None:
            table = view(ITEM_KEY)
        check_item_table(table, None, E, self.device, "dcn_score")
        table = table.detach().contiguous()
        if table.data_ptr() % 16:
            table = table.clone()
        self.n_items = int(table.shape[0])
        self._user_table = view(USER_KEY)
        w0 = view("deep_net.layers.0.linear.weight")
        self._w0u_t = w0[:, :E].t().contiguous()
        self.pi = torch.addmm(view("deep_net.layers.0.linear.bias"), table, w0[:, E:].t()).contiguous()
        self._consts = torch.zeros(2 * _lib.DCN_MAX_CROSS, dtype=torch.float32, device=self.device)
        if self.ln:
            for c in range(self.cross):
                nxt = view(f"cross_net.layers.{c + 1}.weight" if c + 1 < self.cross else "output_layer.weight").reshape(-1)[:2 * E]
                p = f"cross_net.layers.{c}.layer_norm."
                self._consts[c] = (view(p + "weight") * nxt).sum()
                self._consts[_lib.DCN_MAX_CROSS + c] = (view(p + "bias") * nxt).sum()
        self._head = _lib.DcnHeadC(self.factor, self.deep, self.cross, int(self.ln), eps, 0, self.user_num, int(dims[5]), flat.data_ptr(), None)
        self.item_rows = self.rows(table, 1)

    def rows(self, table, half: int):
        """pmgt_dcn_score_rows: the scalars mu, q, d_0 .. d_C of the rows of `table` [rows, E] of `half` (0: users, 1: items)
        -> fp32 [rows, DCN_SCORE_ROW_STRIDE]"""
        import torch
        out = torch.empty(int(table.shape[0]), _lib.DCN_SCORE_ROW_STRIDE, dtype=torch.float32, device=self.device)
        _lib.check(self.lib.pmgt_dcn_score_rows(C.byref(self._head), table.data_ptr(), int(table.shape[0]), half, out.data_ptr(), _lib.stream()))
        return out

    def _launch(self, users, n, out):
        rows = self._user_table.index_select(0, users)
        pu = rows @ self._w0u_t
        user_rows = self.rows(rows, 0)
        _lib.check(self.lib.pmgt_dcn_score(C.byref(self._head), pu.data_ptr(), self.pi.data_ptr(), user_rows.data_ptr(), self.item_rows.data_ptr(),
                                           self._consts.data_ptr(), users.data_ptr(), n, self.n_items, out.data_ptr(), int(out.shape[1]),
                                           _lib.stream()))


class TopkRows:
    """pmgt_topk_rows over score rows of `n_items` live entries, up to `max_rows` rows a call, with an optional exclusion CSR over user ids
    (indptr int64 [user_num + 1], items int32; validated on the host by check_csr).  select(scores, users) -> (items int32 [n, k], scores
    fp32 [n, k], flags uint32 [n]) as device tensors; enqueues one launch, never waits."""

    def __init__(self, device, max_rows: int, n_items: int, k: int, indptr=None, items=None, user_num: int = 0):
        import torch
        self.lib = _lib.hip()
        self.device = torch.device(device)
        self.k, self.max_rows, self.n_items = check_k(k), int(max_rows), int(n_items)
        nbytes = int(self.lib.pmgt_topk_workspace_bytes(self.max_rows, self.n_items))
        if nbytes < 0:
            raise ValueError(f"topk_rows: {max_rows} rows of {n_items} items outside the limits (rows >= 1, items in [1, 2^31 - 2])")
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        self.user_num = int(user_num)
        self._indptr = self._items = None
        if indptr is not None:
            indptr, items = check_csr(indptr, items, self.user_num, self.n_items)
            self._indptr = torch.from_numpy(indptr).to(self.device)
            self._items = torch.from_numpy(items).to(self.device)

    def select(self, scores, users=None, out=None):
        import torch
        n, stride = int(scores.shape[0]), int(scores.shape[1])
        if scores.dtype != torch.float32 or scores.dim() != 2 or not scores.is_contiguous() or scores.device != self._ws.device \
                or not 1 <= n <= self.max_rows or stride < self.n_items:
            raise ValueError(f"topk_rows: scores must be a contiguous fp32 device tensor [1 .. {self.max_rows}, >= {self.n_items}]")
        if self._indptr is not None and (users is None or users.dtype != torch.int64 or tuple(users.shape) != (n,)
                                         or users.device != self._ws.device or not users.is_contiguous()):
            raise ValueError("topk_rows: with an exclusion CSR, users must be a contiguous int64 device tensor [n]")
        if out is None:
            out = (torch.empty(n, self.k, dtype=torch.int32, device=self.device), torch.empty(n, self.k, dtype=torch.float32, device=self.device),
                   torch.empty(n, dtype=torch.int32, device=self.device))
        excl = self._indptr is not None
        _lib.check(self.lib.pmgt_topk_rows(scores.data_ptr(), stride, n, self.n_items, self.k, users.data_ptr() if excl else 0,
                                           self._indptr.data_ptr() if excl else 0, self._items.data_ptr() if excl and len(self._items) else 0,
                                           self.user_num if excl else 0, len(self._items) if excl else 0, self._ws.data_ptr(),
                                           out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), _lib.stream()))
        return out


def select_rows_device(scorer: CatalogueScorer, ids, batch: int, k: int, indptr, excl, id_num: int):
    """The selection pass on the device: per batch of `ids` (int64 numpy, checked by the caller) scorer.score then TopkRows.select, with the
    exclusion CSR (indptr, excl) over `id_num` ids.  Everything is uploaded and built before the first score; nothing is copied to the host
    and nothing waits -> (items int32 [n, k], scores fp32 [n, k], flags int32 [n]) as contiguous DEVICE tensors."""
    import torch
    dev, n, n_items = scorer.device, len(ids), scorer.n_items
    picker = TopkRows(dev, batch, n_items, k, indptr, excl, id_num)
    ids_d = torch.from_numpy(ids).to(dev)
    out = (torch.empty(n, k, dtype=torch.int32, device=dev), torch.empty(n, k, dtype=torch.float32, device=dev),
           torch.empty(n, dtype=torch.int32, device=dev))
    work = torch.empty(batch, n_items, dtype=torch.float32, device=dev)
    for lo in range(0, n, batch):
        hi = min(lo + batch, n)
        scorer.score(ids_d[lo:hi], out=work)
        picker.select(work[: hi - lo], ids_d[lo:hi], out=tuple(t[lo:hi] for t in out))
    return out


def select_device(scorer: CatalogueScorer, ids, batch: int, k: int, indptr, excl, id_num: int):
    """select_rows_device, then one copy at the end fetches -> (items int32 [n, k], scores fp32 [n, k], flags uint32 [n]) as numpy."""
    items, scores, flags = (t.cpu().numpy() for t in select_rows_device(scorer, ids, batch, k, indptr, excl, id_num))      # the copies out: after the loop
    return items, scores, flags.view(np.uint32)


def select_host(score_rows, ids, batch: int, k: int, indptr, excl):
    """The yardstick of select_device: score_rows(ids) -> numpy [m, I] on batches of `ids`, then topk_host; select_device's result."""
    parts = [topk_host(score_rows(ids[lo: lo + batch]), k, indptr, excl, ids[lo: lo + batch]) for lo in range(0, len(ids), batch)]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def default_batch_users(n_users: int, n_items: int) -> int:
    """The largest batch whose [batch, I] fp32 score rows stay within SCORE_WORKSPACE_BYTES (at least one user, at most what one
    pmgt_ncf_score call takes)."""
    return int(max(1, min(n_users, SCORE_WORKSPACE_BYTES // (4 * n_items), NCF_MAX_USERS)))


def host_scores(model, table, users, pair_chunk: int = 1 << 18) -> np.ndarray:
    """impl="host": `model.head` on chunks of (user, item) pair rows gathered from `table`, the full score rows [U, I] copied out."""
    import torch
    dev = table.device
    n_items = int(table.shape[0])
    item_ids = torch.arange(n_items, device=dev)
    per = max(1, pair_chunk // n_items)
    rows = []
    with torch.no_grad():
        for lo in range(0, len(users), per):
            u = torch.from_numpy(np.ascontiguousarray(users[lo: lo + per])).to(dev)
            m = len(u)
            logits = model.head(u[:, None].expand(m, n_items).reshape(-1), item_ids.repeat(m), table.repeat(m, 1))
            rows.append(logits.view(m, n_items).cpu().numpy())
    return np.concatenate(rows)


def dcn_host_scores(model, table, users, pair_chunk: int = 1 << 18) -> np.ndarray:
    """impl="host" for a dcn.DCN: `model.forward` on chunks of (user, item) pair rows, the full score rows [U, I] copied out.  With a
    stand-in `table` the item half of x0 is gathered from it and the rest is forward's own modules (eval mode: no dropout)."""
    import torch
    dev = model.output_layer.weight.device
    n_items = model.item_num
    item_ids = torch.arange(n_items, device=dev)
    per = max(1, pair_chunk // n_items)
    rows = []
    with torch.no_grad():
        for lo in range(0, len(users), per):
            u = torch.from_numpy(np.ascontiguousarray(users[lo: lo + per])).to(dev)
            m = len(u)
            pu, pi = u[:, None].expand(m, n_items).reshape(-1), item_ids.repeat(m)
            if table is None:
                logits = model((pu, pi))
            else:
                x = x0 = torch.cat([model.user_embeddings(pu), table[pi]], dim=-1)
                for layer in model.cross_net.layers:
                    x = layer(x0, x)
                logits = model.output_layer(torch.cat([x, model.deep_net.layers(x0)], dim=-1)).view(-1)
            rows.append(logits.view(m, n_items).cpu().numpy())
    return np.concatenate(rows)


class ModelDispatch:
    """What recommend() and evaluate_catalogue() need to know of the model class, stated once: a PMGT_NCF (encoder + head over an encoded
    catalogue table), the reference's stand-alone NCF class (ncf.py) or a dcn.DCN.  In the caller's order: check_covered() (impl="device":
    the existing check_*_covered of the class), resolve_table() (the default table, check_item_table; sets .dev and .table), then inside
    `with eval_mode(impl):` host_scores(users) or scorer().  `who` names the caller in the messages."""

    def __init__(self, model, who: str):
        from .ncf import NCF
        from .dcn import DCN
        self.model, self.who = model, who
        self.dcn = isinstance(model, DCN)
        self.standalone = isinstance(model, NCF) or self.dcn      # the stand-alone classes: their own tables, no encoder, no sampler
        self.n_items = model.item_num
        self.dev = self.table = None

    def check_covered(self) -> None:
        model = self.model
        if self.dcn:
            check_dcn_covered(model.factor_num, model.deep_layers, model.cross_layers)
        elif self.standalone:
            check_ncf_model_covered(model.factor_num, 1 if model.model == "GMF" else model.num_layers, model.model, model.layer_norm_eps)
        else:
            check_head_covered(model.factor_num, model.num_layers, model.model)

    def resolve_table(self, sampler, table, threads: int, seed: int) -> None:
        model, n_items, who = self.model, self.n_items, self.who
        if self.dcn:
            dev = model.output_layer.weight.device
            if table is not None:
                check_item_table(table, n_items, model.factor_num << model.deep_layers, dev, who)
        elif self.standalone:
            dev = model.predict_layer.weight.device
            if model.model == "GMF":
                if table is not None:
                    raise ValueError(f"{who}: kind 'GMF' reads no item table")
            else:
                if table is None:
                    table = model.embed_item_MLP.weight.detach()
                check_item_table(table, n_items, model.factor_num << (model.num_layers - 1), dev, who)
        else:
            if table is None:
                from .evaluation import encode_catalogue
                with self.eval_mode("host"):
                    table = encode_catalogue(model, sampler, threads=threads, seed=seed)
            dev = model.engine.device
            check_item_table(table, n_items, model.config.hidden_size, dev, who)
        self.dev, self.table = dev, table

    @contextlib.contextmanager
    def eval_mode(self, impl: str):
        """The model in eval mode around the scoring, the mode it had restored behind it (impl="device" on a PMGT_NCF reads the weights
        only: its mode is left alone)."""
        model = self.model
        was_training, set_mode = model.training, impl == "host" or self.standalone
        if set_mode:
            model.eval()
        try:
            yield
        finally:
            if set_mode:
                model.train(was_training)

    def host_scores(self, users) -> np.ndarray:
        """impl="host": the full score rows [U, I] of `users` as numpy."""
        import torch
        if self.dcn:
            return dcn_host_scores(self.model, self.table, users)
        # (kind GMF: model.head ignores the item rows; an empty table carries the item count and the device)
        return host_scores(self.model, torch.empty(self.n_items, 0, device=self.dev) if self.table is None else self.table, users)

    def scorer(self):
        """impl="device": the fused scorer of the class over the resolved table."""
        model = self.model
        if self.dcn:
            from .dcn_train import _flat_of
            return DcnScorer(_flat_of(model, dropout_ok=True), self.table, model.layer_norm_eps)
        if self.standalone:
            return NcfModelScorer(model.state_dict(), self.table, model.model, model.layer_norm_eps)
        return NcfScorer(head_state(model), self.table)


def recommend(model, sampler, users, k: int = 20, exclude=None, batch_users: int = None, impl: str = "device", table=None, threads: int = 8,
              seed: int = 0):
    """For every user of `users`, the k best items of `model`'s whole catalogue (a PMGT_NCF) that are not in the user's exclusion list
    -> (items int64 [U, k], scores fp32 [U, k]) as numpy, best first; ties rank the lower item index first.
    exclude: an iterable of (user, item) pairs, typically the training interactions, or a ready (indptr, items) CSR pair over user ids; it
      is built into the CSR once.  None excludes nothing.
    A user with FEWER THAN k eligible items gets item -1 and score -inf in the slots past them; that is not an error.
    table: a catalogue table of encode_catalogue to reuse; None encodes it once, in eval mode, and restores the caller's train / eval mode.
    batch_users: users per launch; None picks the largest batch whose [batch, I] fp32 score rows stay within 256 MiB.
    impl="device": select_device with the class's fused scorer (pmgt_ncf_score then pmgt_topk_rows per batch).  impl="host": the
      yardstick -- select_host over `model.head` on chunks of pair rows.
    model may also be the reference's stand-alone NCF class (ncf.py; any kind, with or without LayerNorm): `sampler` is then unused (pass
      None), the device is that of the parameters, `table` defaults to model.embed_item_MLP.weight (a trainer's table serves, no copy; kind
      GMF reads none and refuses one), impl="device" is NcfModelScorer + TopkRows in the same loop, and impl="host" on a CPU model needs no GPU.
    model may also be a dcn.DCN: `sampler` is unused, the device is that of the parameters, `table` [I, E] defaults to
      model.item_embeddings.weight (the flat buffer of a DcnTrainer that holds the model is read in place), the model is scored in eval mode
      -- a model with dropout without masks -- and the caller's mode is restored; impl="device" is DcnScorer + TopkRows in the same loop,
      impl="host" is model.forward on chunks of pair rows + topk_host and needs no GPU on a CPU model.
    Raises ValueError for users or excluded ids outside the model's tables, k outside [1, 1024], a user with a NaN score among their
    eligible items (naming how many users), and -- impl="device" only -- a head shape the kernel does not cover."""
    check_impl(impl)
    k = check_k(k)
    users = np.ascontiguousarray(users, dtype=np.int64)
    if users.ndim != 1 or len(users) < 1:
        raise ValueError(f"recommend: users {users.shape} must be [U >= 1]")
    check_ids("users", users, model.user_num, "recommend")
    indptr, excl = exclusion_csr(exclude, model.user_num, model.item_num)
    import torch
    dispatch = ModelDispatch(model, "recommend")
    if impl == "device":
        dispatch.check_covered()
    batch = check_batch(batch_users, len(users), model.item_num, "recommend")
    dispatch.resolve_table(sampler, table, threads, seed)
    with dispatch.eval_mode(impl):
        if impl == "host":
            items, scores, flags = select_host(dispatch.host_scores, users, batch, k, indptr, excl)
        else:
            with torch.no_grad():
                items, scores, flags = select_device(dispatch.scorer(), users, batch, k, indptr, excl, model.user_num)
    refuse_nan("recommend", int(np.count_nonzero(flags & TOPK_FLAG_NAN)), len(users), "users")
    return items.astype(np.int64), scores
