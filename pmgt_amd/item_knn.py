"""The truncated, weighted item-kNN: every item keeps only its m most similar items (build_item_knn: an ItemKnnIndex, built once by the
machinery of similar_items and kept on the device), and a candidate j is scored for user u by the sum, over the items of the user's history
that LIST j among their m neighbours, of their similarity to j, each entry of the history weighted (a rating, a time decay: decay_weights)
or not.  history.py's score lets every item of the catalogue vote with every history item; this is the item-kNN the baselines publish, m
its one hyper-parameter -- and a user costs |H| m gathered entries plus the I floats of the row, whatever d is.

THE SCORE (pmgt_knn_score, ops/knn_score.hip).  H(u) = the user's item ids ascending, no duplicates; w_t the weight of entry t (1 without
weights); nbr / sim the index [I, m], rows best first, -1 / -inf past the end of a short row:
    acc = +0.0
    for t = 0 .. len - 1, in this order:   if j is in the first m live slots of row i_t, at slot c:
        term = sim[i_t][c]                 (no weights)   |   w_t * sim[i_t][c] rounded once to fp32
        acc  = acc + term                  rounded to fp32
    score(u, j) = acc
An item nobody lists scores +0.0 and a zero result is always +0.0.  The bits depend on H(u), its weights and the index rows of its items
alone.  THE ORDER is recommend()'s: descending `score_key`, among equal keys THE LOWER ITEM INDEX FIRST.  Selection, ranks and metrics are
recommend.TopkRows and catalogue_eval.HeldoutRanks / CatalogueMetrics unchanged, through select_device / rank_device.

Not built: the Sarwar normalisation (division by the sum of |sim| of the contributing neighbours), shrinkage, a minimum-similarity cut, a
fused score-and-select that never writes the row.

The pure-numpy part (ItemKnnIndex on numpy arrays, weighted_history_csr, decay_weights, item_knn_scores_host and impl="host") needs no GPU."""
import numpy as np

from . import _lib
from ._lib import NCF_MAX_USERS, TOPK_FLAG_NAN, TOPK_MAX_K
from .catalogue_eval import heldout_csr, heldout_queries, rank_device, rank_host, summarize_catalogue
from .history import HistoryCSR, _exclusion, check_history_users, history_csr, history_entries
from .recommend import (CatalogueScorer, check_batch, check_impl, check_k, refuse_nan, select_device, select_host,
                        select_rows_device)
from .similar import ItemSimScorer, check_metric, check_table, device_table, host_table, item_exclusion_csr, item_sim_host

DEFAULT_M = 64


# ---- host side: pure numpy ------------------------------------------------------------------------------------------------------------------
def check_m(m) -> int:
    if not isinstance(m, (int, np.integer)) or isinstance(m, bool) or not 1 <= int(m) <= TOPK_MAX_K:
        raise ValueError(f"m = {m!r}: expected an integer in [1, {TOPK_MAX_K}]")
    return int(m)


def _is_tensor(x) -> bool:
    return not isinstance(x, np.ndarray) and hasattr(x, "is_cuda")


class ItemKnnIndex:
    """The neighbour index: nbr int32 [I, m] and sim fp32 [I, m], row i = the m neighbours of item i BEST FIRST with their similarities, -1
    / -inf (TopkRows' padding) from the end of a short row on.  Both numpy arrays (a host index) or both contiguous tensors on one GPU (a
    device index); build_item_knn makes one, and ItemKnnIndex(nbr, sim, n_items) takes arrays from elsewhere -- co-review counts, a shrunk
    similarity -- and CHECKS THEM ON THE HOST (tensors are copied out for that): the shapes agree, the ids lie in [-1, n_items), a -1 slot is
    followed only by -1 slots, every value in a live slot is finite, and THE LIVE IDS OF A ROW ARE PAIRWISE DISTINCT, which pmgt_knn_score
    relies on.  `m` = the used columns, `stride` = the columns of the stored rows: truncated(m2) is a view of the first m2 columns (the
    rows are best first, so the index of a smaller m is a prefix of the index of a larger one)."""

    def __init__(self, nbr, sim, n_items: int, _m: int = None, _checked: bool = False):
        if not isinstance(n_items, (int, np.integer)) or isinstance(n_items, bool) or not 1 <= n_items <= 2 ** 31 - 2:
            raise ValueError(f"ItemKnnIndex: n_items = {n_items!r} outside [1, 2^31 - 2]")
        self.n_items = int(n_items)
        self.on_device = _is_tensor(nbr)
        if not _checked:
            if _is_tensor(nbr) != _is_tensor(sim):
                raise ValueError("ItemKnnIndex: nbr and sim must both be numpy arrays or both be tensors")
            if self.on_device:
                if not nbr.is_cuda or nbr.device != sim.device:
                    raise ValueError("ItemKnnIndex: nbr and sim must be tensors on one GPU (or numpy arrays)")
                host_nbr, host_sim = nbr.detach().cpu().numpy(), sim.detach().cpu().numpy()
                nbr, sim = nbr.detach().contiguous(), sim.detach().contiguous()
            else:
                nbr = host_nbr = np.ascontiguousarray(nbr)
                sim = host_sim = np.ascontiguousarray(sim)
            self._check(host_nbr, host_sim)
        self._nbr, self._sim = nbr, sim
        self.stride = int(nbr.shape[1])
        self.m = self.stride if _m is None else int(_m)

    def _check(self, nbr: np.ndarray, sim: np.ndarray) -> None:
        if nbr.ndim != 2 or nbr.shape != sim.shape or nbr.shape[0] != self.n_items or nbr.dtype != np.int32 or sim.dtype != np.float32:
            raise ValueError(f"ItemKnnIndex: nbr {nbr.shape} {nbr.dtype} and sim {sim.shape} {sim.dtype} must be int32 and fp32 "
                             f"[n_items = {self.n_items}, m]")
        check_m(int(nbr.shape[1]))
        if nbr.min() < -1 or nbr.max() >= self.n_items:
            raise ValueError(f"ItemKnnIndex: neighbour ids in [{int(nbr.min())}, {int(nbr.max())}] outside [-1, {self.n_items})")
        live = nbr >= 0
        if (live[:, 1:] & ~live[:, :-1]).any():
            raise ValueError("ItemKnnIndex: a -1 slot must be followed only by -1 slots")
        if not np.isfinite(sim[live]).all():
            raise ValueError(f"ItemKnnIndex: {int(np.count_nonzero(~np.isfinite(sim[live])))} similarities in live slots are not finite")
        ordered = np.sort(nbr, axis=1)
        n_twice = int(np.count_nonzero(((ordered[:, 1:] == ordered[:, :-1]) & (ordered[:, 1:] >= 0)).any(axis=1)))
        if n_twice:
            raise ValueError(f"ItemKnnIndex: {n_twice} of {self.n_items} rows repeat a neighbour id; the live ids of a row must be distinct")

    @property
    def nbr(self):
        """int32 [I, m] (the first m columns of the stored rows: the stored array itself, contiguous, unless truncated)"""
        return self._nbr if self.m == self.stride else self._nbr[:, :self.m]

    @property
    def sim(self):
        """fp32 [I, m]"""
        return self._sim if self.m == self.stride else self._sim[:, :self.m]

    def truncated(self, m2: int) -> "ItemKnnIndex":
        """The index of the m2 <= m best neighbours: a view, nothing is copied or checked again."""
        m2 = check_m(m2)
        if m2 > self.m:
            raise ValueError(f"ItemKnnIndex: m = {m2} is larger than the {self.m} neighbours the index has")
        return ItemKnnIndex(self._nbr, self._sim, self.n_items, _m=m2, _checked=True)

    def host(self) -> "ItemKnnIndex":
        """The same index over numpy arrays (a device index is copied out; a host index is returned as it is)."""
        if not self.on_device:
            return self
        return ItemKnnIndex(self._nbr.cpu().numpy(), self._sim.cpu().numpy(), self.n_items, _m=self.m, _checked=True)

    def device(self, who: str = "ItemKnnIndex") -> "ItemKnnIndex":
        """The same index over device tensors (a host index is uploaded once; a device index is returned as it is)."""
        if self.on_device:
            return self
        import torch
        if not torch.cuda.is_available():
            raise ValueError(f"{who}: impl='device' needs a GPU")
        return ItemKnnIndex(torch.from_numpy(self._nbr).cuda(), torch.from_numpy(self._sim).cuda(), self.n_items, _m=self.m, _checked=True)


def build_item_knn(table, m: int = DEFAULT_M, metric: str = "cosine", batch_items: int = None, impl: str = "device") -> ItemKnnIndex:
    """For every item of `table` [I, d] its m best OTHER items by ItemSimScorer's score (`metric` "cosine" or "dot"), in recommend's order
    -- descending `score_key`, the lower item index first --, item i itself excluded: similar_items over the whole catalogue with k = m,
    the results KEPT ON THE DEVICE (index.nbr int32 [I, m], index.sim fp32 [I, m], contiguous; the only copy to the host is the NaN flags).
    sim[i, c] has the bits of pmgt_item_sim_score.  If I - 1 < m the slots past the end hold -1 / -inf.
    impl="host": the same through select_host over item_sim_host, numpy arrays, no GPU (its sums are BLAS's: not the device's bits).
    batch_items: query items per launch; None picks the largest batch whose [batch, I] fp32 score rows stay within 256 MiB.
    Raises ValueError for m outside [1, 1024], d outside [1, 1024], an unknown metric or impl, and an item with a NaN among its scores
    (naming how many): an index never holds a NaN."""
    who = "build_item_knn"
    check_impl(impl)
    check_metric(metric)
    m = check_m(m)
    n_items, _ = check_table(table, who)
    items = np.arange(n_items, dtype=np.int64)
    indptr, excl = item_exclusion_csr(None, n_items, True)
    batch = check_batch(batch_items, n_items, n_items, who, "batch_items")
    if impl == "host":
        t = host_table(table)
        nbr, sim, flags = select_host(lambda q: item_sim_host(t, q, metric), items, batch, m, indptr, excl)
        n_nan = int(np.count_nonzero(flags & TOPK_FLAG_NAN))
    else:
        import torch
        table_d = device_table(table, who)
        with torch.no_grad(), torch.cuda.device(table_d.device):
            nbr, sim, flags = select_rows_device(ItemSimScorer(table_d, metric), items, batch, m, indptr, excl, n_items)
            n_nan = int(torch.count_nonzero(flags & TOPK_FLAG_NAN))      # the one copy out
    refuse_nan(who, n_nan, n_items, "items")
    return ItemKnnIndex(nbr, sim, n_items, _checked=True)


def weighted_history_csr(histories, weights, n_items: int, user_num: int = None, who: str = "histories"):
    """history_csr with one weight per entry carried through the same sort -> (HistoryCSR (indptr int64 [user_num + 1], items int32), weights
    fp32 aligned with the items): every list ascending by item.  histories: (user, item) integer pairs with weights [len(pairs)], or a
    ready (indptr, items) CSR pair with weights aligned with its items.  A (user, item) pair given twice is REFUSED here (which weight would
    count?); weights must be finite in fp32."""
    owner, items, user_num = history_entries(histories, n_items, user_num, who)
    with np.errstate(over="ignore", invalid="ignore"):
        w = np.asarray(weights, dtype=np.float64).astype(np.float32) if weights is not None else None
    if w is None or w.shape != (len(items),):
        raise ValueError(f"{who}: weights {None if w is None else w.shape} must be [{len(items)}], one per history entry")
    if not np.isfinite(w).all():
        raise ValueError(f"{who}: {int(np.count_nonzero(~np.isfinite(w)))} of {len(w)} weights are not finite in fp32")
    key = owner * np.int64(n_items) + items
    order = np.argsort(key, kind="stable")
    key = key[order]
    n_twice = int(np.count_nonzero(key[1:] == key[:-1]))
    if n_twice:
        raise ValueError(f"{who}: {n_twice} (user, item) pairs are given more than once; with weights every pair must be given once")
    indptr = np.zeros(user_num + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // n_items, minlength=user_num), out=indptr[1:])
    return HistoryCSR((indptr, (key % n_items).astype(np.int32))), np.ascontiguousarray(w[order])


def decay_weights(users, times, half_life) -> np.ndarray:
    """The time-decay weight of every (user, time) entry: 0.5 ** ((t_last(user) - t) / half_life) with t_last the user's LATEST time,
    computed in fp64 and rounded once -> fp32 [P]: a user's latest entry weighs 1, one `half_life` older half of it.  Pure numpy."""
    users = np.asarray(users)
    t = np.asarray(times, dtype=np.float64)
    if users.ndim != 1 or t.shape != users.shape or not np.issubdtype(users.dtype, np.integer):
        raise ValueError(f"decay_weights: users {users.shape} {users.dtype} and times {t.shape} must be one-dimensional, users integer, alike")
    half_life = float(half_life)
    if not (np.isfinite(half_life) and half_life > 0.0):
        raise ValueError(f"decay_weights: half_life = {half_life!r} is not a positive finite number")
    if not np.isfinite(t).all():
        raise ValueError("decay_weights: times must be finite")
    _, slot = np.unique(users, return_inverse=True)
    last = np.full(int(slot.max()) + 1 if len(slot) else 0, -np.inf)
    np.maximum.at(last, slot, t)
    return (0.5 ** ((last[slot] - t) / half_life)).astype(np.float32)


def _history(histories, weights, n_items: int, user_num: int = None):
    """-> (HistoryCSR, weights fp32 aligned with it or None)"""
    if weights is None:
        return history_csr(histories, n_items, user_num), None
    return weighted_history_csr(histories, weights, n_items, user_num)


def _take_index(who: str, index, m):
    """`index` cut to m (None: all it has)"""
    if not isinstance(index, ItemKnnIndex):
        raise ValueError(f"{who}: expected an ItemKnnIndex, got {type(index).__name__}")
    if m is None:
        return index
    m = check_m(m)
    if m > index.m:
        raise ValueError(f"{who}: m = {m} is larger than the {index.m} neighbours the index has")
    return index.truncated(m)


def item_knn_scores_host(index: ItemKnnIndex, histories, users, weights=None, m: int = None) -> np.ndarray:
    """The yardstick of pmgt_knn_score, pure numpy in np.float32, one rounded operation per line -> scores fp32 [U, I] of `users` over the
    index's first m columns (None: all).  Given the same index arrays it equals the kernel bit for bit.  histories: (user, item) pairs or a
    ready (indptr, items) CSR pair, `weights` aligned with them or None.  Refuses a user with an empty history."""
    who = "item_knn_scores_host"
    index = _take_index(who, index, m).host()
    n_items = index.n_items
    (indptr, items), w = _history(histories, weights, n_items)
    users = check_history_users(who, users, indptr)
    nbr, sim = index.nbr, index.sim
    out = np.empty((len(users), n_items), dtype=np.float32)
    for r, u in enumerate(users):
        acc = np.zeros(n_items, dtype=np.float32)            # +0.0
        for t in range(int(indptr[u]), int(indptr[u + 1])):
            i = int(items[t])
            live = (nbr[i] >= 0) & (nbr[i] < n_items)
            ids = nbr[i][live]                               # pairwise distinct: every candidate gets at most one term of this entry
            term = sim[i][live]
            if w is not None:
                term = w[t] * term                           # fp32 * fp32, rounded once
            acc[ids] = acc[ids] + term                       # rounded to fp32
        out[r] = acc
    return out


# ---- device side ------------------------------------------------------------------------------------------------------------------------------
class ItemKnnScorer(CatalogueScorer):
    """pmgt_knn_score over one ItemKnnIndex (a host index is uploaded once; a device index is read in place, its first m columns) and the
    histories of `user_num` users ((user, item) pairs or a ready (indptr, items) CSR pair; `weights` aligned with them, or None):
    ItemKnnScorer(index, histories, user_num) uploads the CSR and the weights once; score(users) launches.  A user with an empty history
    gets a row of NaN (the entry points below refuse such a user first).  Nothing in here copies to the host or waits for the device."""
    entry, ids_name, max_ids, place = "knn_score", "users", NCF_MAX_USERS, "the index's device"

    def __init__(self, index: ItemKnnIndex, histories, user_num: int, weights=None, m: int = None):
        import torch
        index = _take_index("knn_score", index, m)
        if not isinstance(user_num, (int, np.integer)) or isinstance(user_num, bool) or user_num < 1:
            raise ValueError(f"knn_score: user_num = {user_num!r} must be a positive integer")
        self.user_num, self.n_items = int(user_num), index.n_items
        self.history, self.weights = _history(histories, weights, self.n_items, self.user_num)
        self.index = index.device("knn_score")
        self.m = self.index.m
        self.lib = _lib.hip()
        self.device = self.index._nbr.device
        self._indptr = torch.from_numpy(self.history[0]).to(self.device)
        self._items = torch.from_numpy(self.history[1]).to(self.device)
        self._weights = None if self.weights is None else torch.from_numpy(self.weights).to(self.device)

    def _launch(self, users, n, out):
        _lib.check(self.lib.pmgt_knn_score(self.index._nbr.data_ptr(), self.index._sim.data_ptr(), self.index.stride, self.m,
                                           self._indptr.data_ptr(), self._items.data_ptr(),
                                           0 if self._weights is None else self._weights.data_ptr(), users.data_ptr(), n, self.user_num,
                                           self.n_items, out.data_ptr(), int(out.shape[1]), _lib.stream()))


def _resolve(who: str, index_or_table, m):
    """The first argument of the entry points -> (index or None, table or None, n_items, the sizes m asked for as a tuple, whether m came
    as a tuple).  Checks only: a table's index is built by _index_of after every other refusal."""
    many = isinstance(m, (tuple, list))
    ms = tuple(check_m(v) for v in m) if many else (None if m is None else check_m(m),)
    if many and (len(ms) < 1 or any(b <= a for a, b in zip(ms, ms[1:]))):
        raise ValueError(f"{who}: m = {m!r} must be ascending sizes")
    if isinstance(index_or_table, ItemKnnIndex):
        index = index_or_table
        ms = tuple(index.m if v is None else v for v in ms)
        if ms[-1] > index.m:
            raise ValueError(f"{who}: m = {ms[-1]} is larger than the {index.m} neighbours the index has")
        return index, None, index.n_items, ms, many
    n_items, _ = check_table(index_or_table, who)
    return None, index_or_table, n_items, tuple(DEFAULT_M if v is None else v for v in ms), many


def _index_of(index, table, m: int, batch_items, impl: str, who: str) -> ItemKnnIndex:
    """the index at m columns on the side `impl` runs on: taken (moved if it lives on the other side) or built from the table"""
    if index is None:
        index = build_item_knn(table, m, "cosine", batch_items, impl)
    return index.truncated(m).host() if impl == "host" else index.truncated(m).device(who)


def recommend_item_knn(index_or_table, histories, users=None, k: int = 20, m=None, weights=None, exclude="history", batch_users: int = None,
                       impl: str = "device"):
    """For every user of `users` (None: every user with a history, ascending), the k items of the whole catalogue that score best against
    the user's history under the truncated, weighted item-kNN score of this module and are not in the user's exclusion list
    -> (items int64 [U, k], scores fp32 [U, k]) as numpy, best first; ties rank the lower item index first: recommend()'s order and padding
    (a user with FEWER THAN k eligible items gets item -1 and score -inf in the slots past them; that is not an error).
    index_or_table: an ItemKnnIndex (m None: all its neighbours; else its first m), or a table [I, d] fp32 as recommend_from_history takes
      it, whose index is built first with m neighbours (None: 64) under the cosine, on the side `impl` names.
    histories, exclude, batch_users: recommend_from_history's.  weights: one per history entry, aligned with `histories` (pairs or a CSR
      pair): a (user, item) pair given twice is then refused; None weighs every entry 1 and a pair given twice counts once.
    impl="device": recommend.select_device with an ItemKnnScorer.  impl="host": the yardstick -- select_host over item_knn_scores_host.
    Raises ValueError for a queried user with an empty history, ids outside the table or the CSR, k or m outside [1, 1024], m larger than
    the index has, weights of the wrong length or not finite, duplicate pairs given with weights, an unknown impl, and a user with a NaN
    score among their eligible items (naming how many)."""
    who = "recommend_item_knn"
    check_impl(impl)
    k = check_k(k)
    if isinstance(m, (tuple, list)):
        raise ValueError(f"{who}: m must be one size (evaluate_item_knn takes several)")
    index, table, n_items, (m,), _ = _resolve(who, index_or_table, m)
    history, w = _history(histories, weights, n_items)
    user_num = len(history[0]) - 1
    users = check_history_users(who, np.nonzero(np.diff(history[0]) > 0)[0] if users is None else users, history[0])
    indptr, excl = _exclusion(exclude, history, n_items)
    batch = check_batch(batch_users, len(users), n_items, who)
    index = _index_of(index, table, m, None, impl, who)
    if impl == "host":
        found, scores, flags = select_host(lambda u: item_knn_scores_host(index, history, u, w), users, batch, k, indptr, excl)
    else:
        import torch
        with torch.no_grad(), torch.cuda.device(index._nbr.device):
            found, scores, flags = select_device(ItemKnnScorer(index, history, user_num, w), users, batch, k, indptr, excl, user_num)
    refuse_nan(who, int(np.count_nonzero(flags & TOPK_FLAG_NAN)), len(users), "users")
    return found.astype(np.int64), scores


def evaluate_item_knn(index_or_table, histories, heldout, ks=(10, 20), m=None, weights=None, exclude="history", batch_users: int = None,
                      impl: str = "device", per_user: bool = False):
    """Whole-catalogue quality of the truncated item-kNN recommender on held-out (user, item) pairs -> evaluate_catalogue's dictionary
    {"n<k>", "r<k>", "hr<k>" for k in ks, "mrr", "users", "pairs"}: every user with a held-out item ranks ALL items of the catalogue outside
    their exclusion list by recommend_item_knn's score, in its order.
    m: one size as in recommend_item_knn, or a TUPLE of ascending sizes: then ONE index is built (or taken) at the largest and the result
      is {m_i: dictionary}, each entry scored on index.truncated(m_i) -- a sweep over the one hyper-parameter of the model.
    index_or_table, histories, weights, exclude, batch_users, impl: recommend_item_knn's; heldout, ks, per_user: evaluate_history's
      (per_user=True: (result, dict) in the place of every dictionary).
    Raises ValueError for what recommend_item_knn refuses and for a held-out pair that is also excluded (naming how many) and an empty
    held-out set."""
    from .metrics import check_ks
    who = "evaluate_item_knn"
    check_impl(impl)
    ks = check_ks(ks)
    index, table, n_items, ms, many = _resolve(who, index_or_table, m)
    history, w = _history(histories, weights, n_items)
    user_num = len(history[0]) - 1
    held = heldout_csr(heldout, user_num, n_items)
    exclusion, users = heldout_queries(who, held, lambda: _exclusion(exclude, history, n_items), n_items)
    users = check_history_users(who, users, history[0])
    batch = check_batch(batch_users, len(users), n_items, who)
    index = _index_of(index, table, ms[-1], None, impl, who)
    results = {}
    for mi in ms:
        cut = index.truncated(mi)
        if impl == "host":
            sums, rec, ranks = rank_host(lambda u: item_knn_scores_host(cut, history, u, w), users, batch, held, exclusion, ks)
        else:
            import torch
            with torch.no_grad(), torch.cuda.device(cut._nbr.device):
                sums, rec, ranks = rank_device(ItemKnnScorer(cut, history, user_num, w), users, batch, held, exclusion, user_num, ks, per_user)
        refuse_nan(who, sums["n_nan"], len(users), "users")
        result = summarize_catalogue(sums, len(users), len(held[1]), ks)
        if per_user:
            rec.update(ranks=ranks, indptr=held[0], items=held[1])
            result = (result, rec)
        results[mi] = result
    return results if many else results[ms[0]]
