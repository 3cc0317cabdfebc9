"""Recommending from a user's history (item-kNN over the embeddings): item j is scored for user u by how similar it is to the items the user
already has, score(u, j) = agg over i in H(u) of s(i, j), with s the item-by-item score of similar.py (the cosine or the dot product of two
rows of ONE table -- the encoder's CLS vectors) and H(u) the user's history.  It needs no trained head and no row of a user table: a user
who arrived after training is served from their history alone (recommend_from_history), and a pre-trained encoder is judged on the
downstream task, whole catalogue, before any head exists (evaluate_history) -- the head-free baseline of a fit_ncf / fit_dcn result.

THE SCORE (pmgt_history_score, ops/history_score.hip).  H(u) = the user's item ids ascending, duplicates dropped; s(i, j) has the bits of
pmgt_item_sim_score.
  agg "max":   the largest s(i, j) over H(u); NaN if any term is NaN; a zero result is +0.0
  agg "mean":  acc = s(i_0, j), then acc = acc + s(i_t, j) in ascending item id, every sum rounded to fp32; score = acc / float(len)
The bits depend on H(u), the rows of its items and row j alone: not on the batch, the user's slot in it, or how the catalogue is cut.
THE ORDER is recommend()'s: descending `score_key`, among equal keys THE LOWER ITEM INDEX FIRST.  Selection, ranks and metrics are
recommend.TopkRows and catalogue_eval.HeldoutRanks / CatalogueMetrics unchanged, through select_device / rank_device.

The pure-numpy part (history_csr, history_scores_host and impl="host") needs no GPU."""
import numpy as np

from . import _lib
from ._lib import HISTORY_AGGS, NCF_MAX_USERS, TOPK_FLAG_NAN
from .catalogue_eval import heldout_csr, heldout_queries, rank_device, rank_host, summarize_catalogue
from .pair_train import check_ids
from .recommend import CatalogueScorer, check_batch, check_csr, check_impl, check_k, exclusion_csr, refuse_nan, select_device, select_host
from .similar import check_metric, check_table, device_table, host_table, item_sim_host


# ---- host side: pure numpy ------------------------------------------------------------------------------------------------------------------
def check_agg(agg) -> str:
    if agg not in HISTORY_AGGS:
        raise ValueError(f"agg={agg!r}: expected 'mean' or 'max'")
    return agg


class HistoryCSR(tuple):
    """(indptr, items) as history_csr built it: validated, every list ascending without duplicates.  history_csr hands one back as it is, so
    a driver builds the CSR once and passes it through the scorer and the yardstick."""


def is_csr_pair(x) -> bool:
    """a ready (indptr, items) pair: a tuple of two one-dimensional numpy arrays (pairs come as one [n, 2] array or an iterable of 2-tuples)"""
    return isinstance(x, tuple) and len(x) == 2 and all(isinstance(a, np.ndarray) and a.ndim == 1 for a in x)


def history_entries(histories, n_items: int, user_num: int = None, who: str = "histories"):
    """The validated entries of `histories` ((user, item) integer pairs or a ready (indptr, items) pair) IN THE ORDER GIVEN
    -> (owner int64 [P], items int64 [P], user_num); user_num None: the CSR's own length, or the largest user id of the pairs plus one."""
    if is_csr_pair(histories):
        if user_num is None:
            user_num = len(histories[0]) - 1
        if user_num < 1:
            raise ValueError(f"{who}: indptr {histories[0].shape} must be [user_num + 1] with user_num >= 1")
        indptr, items = check_csr(histories[0], histories[1], user_num, n_items, who, "history items")
        owner = np.repeat(np.arange(user_num, dtype=np.int64), np.diff(indptr))
        items = items.astype(np.int64)
    else:
        pairs = np.asarray(histories if isinstance(histories, np.ndarray) else list(histories if histories is not None else ()))
        if pairs.size == 0:
            raise ValueError(f"{who}: no history at all")
        if pairs.ndim != 2 or pairs.shape[1] != 2 or not np.issubdtype(pairs.dtype, np.integer):
            raise ValueError(f"{who}: expected (user, item) integer pairs, got an array of shape {pairs.shape} and dtype {pairs.dtype}")
        pairs = pairs.astype(np.int64)
        if user_num is None:
            user_num = int(max(pairs[:, 0].max(), 0)) + 1
        check_ids("users", pairs[:, 0], user_num, who)
        check_ids("history items", pairs[:, 1], n_items, who)
        owner, items = pairs[:, 0], pairs[:, 1]
    if len(items) < 1:
        raise ValueError(f"{who}: no history at all")
    return owner, items, user_num


def history_csr(histories, n_items: int, user_num: int = None, who: str = "histories"):
    """The history CSR over user ids from (user, item) integer pairs or a ready (indptr, items) pair -> (indptr int64 [user_num + 1], items
    int32), every list ASCENDING by item with DUPLICATES DROPPED: the order of the pairs does not matter and a pair given twice counts once.
    user_num None: the CSR's own length, or the largest user id of the pairs plus one.  A HistoryCSR (this function's own result) over the
    same ids is returned as it is."""
    if isinstance(histories, HistoryCSR) and user_num in (None, len(histories[0]) - 1) and int(histories[1].max()) < n_items:
        return histories
    owner, items, user_num = history_entries(histories, n_items, user_num, who)
    key = np.unique(owner * np.int64(n_items) + items)
    indptr = np.zeros(user_num + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // n_items, minlength=user_num), out=indptr[1:])
    return HistoryCSR((indptr, (key % n_items).astype(np.int32)))


def check_history_users(who: str, users, indptr) -> np.ndarray:
    """`users` as int64 [U >= 1]; ValueError in the name of `who` for an id outside the CSR and for a user whose history is empty"""
    users = np.ascontiguousarray(users, dtype=np.int64)
    if users.ndim != 1 or len(users) < 1:
        raise ValueError(f"{who}: users {users.shape} must be [U >= 1]")
    check_ids("users", users, len(indptr) - 1, who)
    n_empty = int(np.count_nonzero(np.diff(indptr)[users] == 0))
    if n_empty:
        raise ValueError(f"{who}: {n_empty} of {len(users)} users have an empty history")
    return users


def reduce_history(rows: np.ndarray, agg: str) -> np.ndarray:
    """THE REDUCTION of the item scores `rows` [len >= 1, I] of one user's history items (ascending item id) -> [I], in the dtype of rows"""
    if agg == "max":
        with np.errstate(invalid="ignore"):
            m = rows.max(axis=0)                             # (numpy's max keeps a NaN)
        return np.where(m == 0, rows.dtype.type(0), m)       # a zero result is +0.0
    acc = rows[0].copy()
    for t in range(1, len(rows)):
        acc = acc + rows[t]                                  # one rounded sum after the other, ascending item id
    return acc / rows.dtype.type(len(rows))


def history_scores_host(table, histories, users, agg: str = "mean", metric: str = "cosine", eps: float = 1e-12, dtype=np.float32) -> np.ndarray:
    """The yardstick of pmgt_history_score, pure numpy in `dtype`: scores [U, I] of `users` against every row of `table` [I, d] -- per user
    item_sim_host's rows of the history items, then the reduction exactly as the module states it.  histories: (user, item) pairs or a ready
    (indptr, items) CSR pair.  Refuses a user with an empty history."""
    check_agg(agg)
    check_metric(metric)
    t = np.ascontiguousarray(host_table(table), dtype=dtype)
    if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"history_scores_host: table {t.shape} must be [I >= 1, d >= 1]")
    indptr, items = history_csr(histories, t.shape[0])
    users = check_history_users("history_scores_host", users, indptr)
    out = np.empty((len(users), t.shape[0]), dtype=dtype)
    for r, u in enumerate(users):
        out[r] = reduce_history(item_sim_host(t, items[indptr[u]: indptr[u + 1]], metric, eps, dtype), agg)
    return out


# ---- device side ------------------------------------------------------------------------------------------------------------------------------
class HistoryScorer(CatalogueScorer):
    """pmgt_history_score over one table [I, d] (fp32, contiguous, on a GPU), read in place, and the histories of `user_num` users ((user, item)
    pairs or a ready (indptr, items) CSR pair): HistoryScorer(table, histories, user_num) computes the inverse norms once
    (pmgt_item_sim_norms; metric "dot" has none) and uploads the history CSR once; score(users) launches.  A user with an empty history gets
    a row of NaN (the entry points below refuse such a user first).  Nothing in here copies to the host or waits for the device."""
    entry, ids_name, max_ids = "history_score", "users", NCF_MAX_USERS

    def __init__(self, table, histories, user_num: int, agg: str = "mean", metric: str = "cosine", eps: float = 1e-12):
        import torch
        self.agg, self.metric = check_agg(agg), check_metric(metric)
        self.n_items, self.d = check_table(table, "history_score")
        if not isinstance(table, torch.Tensor) or not table.is_cuda or not table.is_contiguous():
            raise ValueError("history_score: the table must be a contiguous fp32 tensor on a GPU")
        eps = float(np.float32(eps))
        if not (np.isfinite(eps) and eps > 0.0):
            raise ValueError(f"history_score: eps = {eps!r} is not a positive finite number")
        if not isinstance(user_num, (int, np.integer)) or isinstance(user_num, bool) or user_num < 1:
            raise ValueError(f"history_score: user_num = {user_num!r} must be a positive integer")
        self.user_num = int(user_num)
        self.history = history_csr(histories, self.n_items, self.user_num)
        self.lib = _lib.hip()
        self.table = table.detach()
        self.device = table.device
        self._indptr = torch.from_numpy(self.history[0]).to(self.device)
        self._items = torch.from_numpy(self.history[1]).to(self.device)
        self.inv_norm = None
        if metric == "cosine":
            self.inv_norm = torch.empty(self.n_items, dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(self.lib.pmgt_item_sim_norms(self.table.data_ptr(), self.n_items, self.d, eps, self.inv_norm.data_ptr(), _lib.stream()))

    def _launch(self, users, n, out):
        _lib.check(self.lib.pmgt_history_score(self.table.data_ptr(), 0 if self.inv_norm is None else self.inv_norm.data_ptr(),
                                               self._indptr.data_ptr(), self._items.data_ptr(), users.data_ptr(), n, self.user_num, self.n_items,
                                               self.d, HISTORY_AGGS.index(self.agg), out.data_ptr(), int(out.shape[1]), _lib.stream()))


def _exclusion(exclude, history, n_items: int):
    """exclude="history": what the user already has; else recommend's: None, (user, item) pairs or a ready CSR pair"""
    if isinstance(exclude, str):
        if exclude != "history":
            raise ValueError(f"exclude={exclude!r}: expected 'history', None, (user, item) pairs or an (indptr, items) pair")
        return history
    return exclusion_csr(exclude, len(history[0]) - 1, n_items)


def recommend_from_history(table, histories, users=None, k: int = 20, agg: str = "mean", metric: str = "cosine", exclude="history",
                           batch_users: int = None, impl: str = "device"):
    """For every user of `users` (None: every user with a history, ascending), the k items of the whole catalogue that score best against
    the user's history under `agg` ("mean" or "max") of `metric` ("cosine" or "dot") and are not in the user's exclusion list
    -> (items int64 [U, k], scores fp32 [U, k]) as numpy, best first; ties rank the lower item index first: recommend()'s order and padding
    (a user with FEWER THAN k eligible items gets item -1 and score -inf in the slots past them; that is not an error).
    table: [I, d] fp32 -- the device tensor encode_catalogue returns, or a numpy array such as export_embeddings returns (impl="device"
      uploads it once); read in place, never normalised.
    histories: (user, item) integer pairs or a ready (indptr, items) CSR pair over user ids; a pair given twice counts once and the order
      of the pairs does not matter.  The user ids run to the CSR's length, or to the largest user of the pairs.
    exclude: "history" excludes what the user already has; None, (user, item) pairs or a ready CSR pair are taken as recommend() takes them.
    batch_users: users per launch; None picks the largest batch whose [batch, I] fp32 score rows stay within 256 MiB.
    impl="device": recommend.select_device with a HistoryScorer.  impl="host": the yardstick -- select_host over history_scores_host; no GPU.
    Raises ValueError for a queried user with an empty history, ids outside the table or the CSR, an unknown agg, metric or impl, k outside
    [1, 1024], d outside [1, 1024], and a user with a NaN score among their eligible items (naming how many)."""
    who = "recommend_from_history"
    check_impl(impl)
    check_agg(agg)
    check_metric(metric)
    k = check_k(k)
    n_items, _ = check_table(table, who)
    history = history_csr(histories, n_items)
    user_num = len(history[0]) - 1
    users = check_history_users(who, np.nonzero(np.diff(history[0]) > 0)[0] if users is None else users, history[0])
    indptr, excl = _exclusion(exclude, history, n_items)
    batch = check_batch(batch_users, len(users), n_items, who)
    if impl == "host":
        t = host_table(table)
        found, scores, flags = select_host(lambda u: history_scores_host(t, history, u, agg, metric), users, batch, k, indptr, excl)
    else:
        import torch
        table_d = device_table(table, who)
        with torch.no_grad(), torch.cuda.device(table_d.device):
            found, scores, flags = select_device(HistoryScorer(table_d, history, user_num, agg, metric), users, batch, k, indptr, excl, user_num)
    refuse_nan(who, int(np.count_nonzero(flags & TOPK_FLAG_NAN)), len(users), "users")
    return found.astype(np.int64), scores


def evaluate_history(table, histories, heldout, ks=(10, 20), agg: str = "mean", metric: str = "cosine", exclude="history",
                     batch_users: int = None, impl: str = "device", per_user: bool = False):
    """Whole-catalogue quality of the embeddings `table` [I, d] as an item-kNN recommender on held-out (user, item) pairs ->
    evaluate_catalogue's dictionary {"n<k>", "r<k>", "hr<k>" for k in ks, "mrr", "users", "pairs"}.  Every user with a held-out item ranks
    ALL items of the catalogue outside their exclusion list by recommend_from_history's score, in its order, and the metrics say where the
    held-out items land.  No head is trained: this is the baseline a fit_ncf / fit_dcn result is compared against.
    heldout: (user, item) pairs or a ready CSR pair over the histories' user ids; duplicates are dropped.  The evaluated users are those
      with at least one held-out item, ascending; each needs a history.
    table, histories, agg, metric, exclude, batch_users: recommend_from_history's.  impl="device": catalogue_eval.rank_device with a
      HistoryScorer.  impl="host": the yardstick -- rank_host over history_scores_host; needs no GPU.
    per_user=True: returns (result, dict) with users, n_pos, ndcg[k], recall[k], hit[k], rr per evaluated user, and ranks with the held-out
      CSR (indptr, items) they align with.
    Raises ValueError for an evaluated user with an empty history, ids outside the table or the CSR, a held-out pair that is also excluded
    (naming how many), an empty held-out set, an unknown agg, metric or impl, d outside [1, 1024], and a user with a NaN score among their
    eligible items (naming how many)."""
    from .metrics import check_ks
    who = "evaluate_history"
    check_impl(impl)
    check_agg(agg)
    check_metric(metric)
    ks = check_ks(ks)
    n_items, _ = check_table(table, who)
    history = history_csr(histories, n_items)
    user_num = len(history[0]) - 1
    held = heldout_csr(heldout, user_num, n_items)
    exclusion, users = heldout_queries(who, held, lambda: _exclusion(exclude, history, n_items), n_items)
    users = check_history_users(who, users, history[0])
    batch = check_batch(batch_users, len(users), n_items, who)
    if impl == "host":
        t = host_table(table)
        sums, rec, ranks = rank_host(lambda u: history_scores_host(t, history, u, agg, metric), users, batch, held, exclusion, ks)
    else:
        import torch
        table_d = device_table(table, who)
        with torch.no_grad(), torch.cuda.device(table_d.device):
            sums, rec, ranks = rank_device(HistoryScorer(table_d, history, user_num, agg, metric), users, batch, held, exclusion, user_num, ks,
                                           per_user)
    refuse_nan(who, sums["n_nan"], len(users), "users")
    result = summarize_catalogue(sums, len(users), len(held[1]), ks)
    if not per_user:
        return result
    rec.update(ranks=ranks, indptr=held[0], items=held[1])
    return result, rec
