"""Evaluation on the whole catalogue: for every held-out (user, item) pair the exact place of the item among the items the user may be
recommended, and nDCG@k / Recall@k / HR@k / MRR from those places -- the quality of what recommend() returns.  The reference evaluates on
positives plus sampled negatives (pmgt/ncf/trainer.py:202-254; evaluate_ranking restates that); sampled metrics are known to disagree with
whole-catalogue ones, even about which of two models is better.  Here the reference's get_ndcg / get_recall (pmgt/metrics.py:16-37) are
applied to each user's whole-catalogue list, which is never built: a rank says where an item is however far down, a top-k is blind beyond k.

THE ORDER is recommend()'s: descending `score_key`, among equal keys THE LOWER ITEM INDEX FIRST.  With the composite
c(j) = key(j) << 32 | (0xFFFFFFFF - j), distinct for every item of a row,
      rank(u, p) = 1 + #{ j eligible for u, j != p : c(j) > c(p) }
is the 1-based place of p in recommend(..., k = everything); the user's other held-out items count like any item.

The pure-numpy part (heldout_csr, heldout_ranks_host, catalogue_metrics_host) needs no GPU; the device part is pmgt_rank_heldout and
pmgt_rank_heldout_reduce (ops/catalogue_rank.hip) behind HeldoutRanks and CatalogueMetrics."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import NCF_MAX_USERS, RANK_HELDOUT_CHUNK, RANK_HELDOUT_FLAG_EXCLUDED, RANK_HELDOUT_HEADER_BYTES, TOPK_FLAG_NAN  # noqa: F401
from .evaluation import score_key
from .metrics import RANK_MAX_KS      # PMGT_RANK_MAX_KS: the header holds that many sums a quantity
from .recommend import ModelDispatch, check_batch, check_csr, check_impl, default_batch_users, exclusion_csr, refuse_nan  # noqa: F401

SUM_THREADS = 256             # the threads of the fixed summation tree


# ---- host side: pure numpy ------------------------------------------------------------------------------------------------------------------
def heldout_csr(heldout, user_num: int, item_num: int):
    """The held-out CSR over user ids from an iterable of (user, item) pairs or a ready (indptr, items) pair, validated as exclusion_csr
    validates an exclusion list (its messages, in the held-out set's name) -> (indptr int64 [user_num + 1], items int32), every list
    sorted by item with DUPLICATES DROPPED."""
    indptr, items = exclusion_csr(heldout, user_num, item_num, "heldout", "held-out items")
    owner = np.repeat(np.arange(user_num, dtype=np.int64), np.diff(indptr))
    pair = np.unique(owner * np.int64(item_num) + items.astype(np.int64))
    out = np.zeros(user_num + 1, dtype=np.int64)
    np.cumsum(np.bincount(pair // item_num, minlength=user_num), out=out[1:])
    return out, (pair % item_num).astype(np.int32)


def count_common_pairs(a_csr, b_csr, item_num: int) -> int:
    """How many distinct (user, item) pairs two CSRs over the same user ids share."""
    ids = []
    for indptr, items in (a_csr, b_csr):
        owner = np.repeat(np.arange(len(indptr) - 1, dtype=np.int64), np.diff(indptr))
        ids.append(np.unique(owner * np.int64(item_num) + np.asarray(items, dtype=np.int64)))
    return int(len(np.intersect1d(ids[0], ids[1], assume_unique=True)))


def heldout_queries(who: str, heldout, build_exclusion, n_items: int):
    """The held-out prelude of evaluate_catalogue and evaluate_neighbours, in their order of refusals: an empty held-out CSR `heldout` is
    refused, then build_exclusion() builds (and validates) the exclusion CSR, then a held-out pair that is also excluded is refused
    -> (the exclusion CSR, the evaluated ids: those with at least one held-out item, ascending)."""
    n_pairs = len(heldout[1])
    if n_pairs < 1:
        raise ValueError(f"{who}: the held-out set is empty")
    exclusion = build_exclusion()
    n_both = count_common_pairs(heldout, exclusion, n_items)
    if n_both:
        raise ValueError(f"{who}: {n_both} of {n_pairs} held-out pairs are also excluded")
    return exclusion, np.nonzero(np.diff(heldout[0]) > 0)[0].astype(np.int64)


def heldout_ranks_host(scores, users, heldout_csr, exclusion_csr=None):
    """The yardstick of pmgt_rank_heldout, pure numpy.  scores [n, I] (row r is user users[r]'s), heldout_csr = (indptr int64
    [user_num + 1], items int32), exclusion_csr the same or None (everything is eligible).
    -> (ranks int32 [len(held-out items)], aligned with the held-out CSR; flags uint32 [n]).  ranks[h] = 1 + the number of eligible items
    of the user whose composite is above the held-out item's; a held-out item that is also excluded gets 0 and sets flag bit 2
    (RANK_HELDOUT_FLAG_EXCLUDED); a NaN among the row's eligible scores sets bit 0 (TOPK_FLAG_NAN).  A row whose user has no held-out item
    leaves its flag 0; places of the held-out CSR that no row reaches stay 0."""
    x = np.ascontiguousarray(scores, dtype=np.float32)
    if x.ndim != 2 or x.shape[1] < 1:
        raise ValueError(f"heldout_ranks_host: scores {x.shape} must be [n, I] with I >= 1")
    n, n_items = x.shape
    users = np.asarray(users, dtype=np.int64)
    if users.shape != (n,):
        raise ValueError(f"heldout_ranks_host: users {users.shape} must be [n = {n}]")
    h_indptr, h_items = heldout_csr
    ranks = np.zeros(len(h_items), dtype=np.int32)
    flags = np.zeros(n, dtype=np.uint32)
    low = np.uint64(0xFFFFFFFF) - np.arange(n_items, dtype=np.uint64)
    for r in range(n):
        u = users[r]
        lo, hi = int(h_indptr[u]), int(h_indptr[u + 1])
        if hi <= lo:
            continue
        c = (score_key(x[r]).astype(np.uint64) << np.uint64(32)) | low
        eligible = np.ones(n_items, dtype=bool)
        if exclusion_csr is not None:
            eligible[np.asarray(exclusion_csr[1][exclusion_csr[0][u]: exclusion_csr[0][u + 1]], dtype=np.int64)] = False
        above = np.sort(c[eligible])
        held = np.asarray(h_items[lo:hi], dtype=np.int64)
        ok = eligible[held]
        ranks[lo:hi] = np.where(ok, len(above) - np.searchsorted(above, c[held], side="right") + 1, 0)
        flags[r] = np.uint32((np.isnan(x[r]) & eligible).any() * TOPK_FLAG_NAN + (not ok.all()) * RANK_HELDOUT_FLAG_EXCLUDED)
    return ranks, flags


def tree_sum_host(values) -> float:
    """The fixed summation order of the device reduce in numpy: part t of 256 adds values[t], values[t + 256], ... in ascending order, the 64
    parts of a wave are folded by a butterfly (distance 32, 16, .., 1), the four wave sums are added in order."""
    v = np.ascontiguousarray(values, dtype=np.float64)
    part = np.zeros(SUM_THREADS, dtype=np.float64)
    for t in range(min(SUM_THREADS, len(v))):
        part[t] = np.cumsum(v[t::SUM_THREADS])[-1]           # (cumsum adds one after the other)
    w = part.reshape(SUM_THREADS // 64, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[:, lane ^ o]
    return float(((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0])


def catalogue_metrics_host(ranks, indptr, ks=(10, 20)) -> dict:
    """The yardstick of pmgt_rank_heldout_reduce, pure numpy, the arithmetic of ranking_metrics_host: per user with n_pos held-out items
    (the users with at least one, in ascending id order) recall_k = #{rank <= k} / n_pos, dcg_k = the discounts 1 / log2(rank + 1) of the
    ranks <= k added in ascending rank in fp64, ndcg_k = dcg_k / idcg[min(n_pos, k) - 1], hit_k = (min rank <= k), rr = 1 / min rank; rank 0
    is no rank.  ranks int32 aligned with the CSR whose indptr is given.
    -> dict: users int64 [U]; n_pos int64 [U]; ndcg[k], recall[k], hit[k], rr fp64 [U]; sums = {"ndcg": {k}, "recall": {k}, "hit": {k},
    "rr"} over the users in the device's fixed order (tree_sum_host)."""
    from .metrics import check_ks, discount_tables
    ks = check_ks(ks)
    indptr = np.asarray(indptr, dtype=np.int64)
    ranks = np.asarray(ranks, dtype=np.int64)
    counts = np.diff(indptr)
    if indptr.ndim != 1 or len(indptr) < 2 or indptr[0] != 0 or (counts < 0).any() or indptr[-1] != len(ranks):
        raise ValueError("catalogue_metrics_host: indptr must be non-decreasing from 0 to len(ranks)")
    users = np.nonzero(counts > 0)[0].astype(np.int64)
    if len(users) < 1:
        raise ValueError("catalogue_metrics_host: no held-out item")
    U, max_k = len(users), ks[-1]
    n_pos = counts[users]
    owner = np.repeat(np.arange(U), n_pos)                   # every place of the CSR belongs to one of these users, in order
    disc, idcg = discount_tables(max_k)
    hit = np.zeros((U, max_k), dtype=bool)
    top = (ranks >= 1) & (ranks <= max_k)
    hit[owner[top], ranks[top] - 1] = True
    best = np.full(U, np.iinfo(np.int64).max, dtype=np.int64)
    np.minimum.at(best, owner[ranks >= 1], ranks[ranks >= 1])
    dcg = np.cumsum(np.where(hit, disc[None, :], 0.0), axis=1)      # sequential along the rank: the adds in ascending order
    nhit = np.cumsum(hit, axis=1)
    out = dict(users=users, n_pos=n_pos, ndcg={}, recall={}, hit={})
    for k in ks:
        out["recall"][k] = nhit[:, k - 1].astype(np.float64) / n_pos.astype(np.float64)
        out["ndcg"][k] = dcg[:, k - 1] / idcg[np.minimum(n_pos, k) - 1]
        out["hit"][k] = (best <= k).astype(np.float64)
    ranked = best != np.iinfo(np.int64).max
    out["rr"] = np.where(ranked, 1.0 / np.where(ranked, best, 1).astype(np.float64), 0.0)
    out["sums"] = dict(ndcg={k: tree_sum_host(out["ndcg"][k]) for k in ks}, recall={k: tree_sum_host(out["recall"][k]) for k in ks},
                       hit={k: tree_sum_host(out["hit"][k]) for k in ks}, rr=tree_sum_host(out["rr"]))
    return out


def rank_host(score_rows, ids, batch: int, heldout, exclusion, ks):
    """The yardstick of rank_device: score_rows(ids) -> numpy [m, I] on batches of `ids`, heldout_ranks_host, then catalogue_metrics_host;
    rank_device's result with the records always there."""
    ranks = np.zeros(len(heldout[1]), dtype=np.int32)
    flags = np.zeros(len(ids), dtype=np.uint32)
    for lo in range(0, len(ids), batch):
        q = ids[lo: lo + batch]
        r, flags[lo: lo + batch] = heldout_ranks_host(score_rows(q), q, heldout, exclusion)
        ranks = np.maximum(ranks, r)                         # (a call fills the places of its own ids, the others stay 0)
    records = catalogue_metrics_host(ranks, heldout[0], ks)
    sums = records.pop("sums")
    sums["n_nan"] = int(np.count_nonzero(flags & TOPK_FLAG_NAN))
    return sums, records, ranks


def summarize_catalogue(sums: dict, n_users: int, n_pairs: int, ks) -> dict:
    """{"n<k>", "r<k>", "hr<k>" for k in ks, "mrr", "users", "pairs"}: the means over the evaluated users from their sums."""
    n = float(n_users)
    out = {f"n{k}": sums["ndcg"][k] / n for k in ks}
    out.update({f"r{k}": sums["recall"][k] / n for k in ks})
    out.update({f"hr{k}": sums["hit"][k] / n for k in ks})
    out.update(mrr=sums["rr"] / n, users=int(n_users), pairs=int(n_pairs))
    return out


# ---- device side ------------------------------------------------------------------------------------------------------------------------------
class HeldoutRanks:
    """pmgt_rank_heldout over score rows of `n_items` live entries: owns the uploaded held-out CSR (validated on the host by check_csr), the
    optional exclusion CSR and the ranks int32 [len(held-out items)], zero until a row of the item's user is ranked.
    rank(scores, users) -> (ranks, flags uint32 [n] as an int32 device tensor); enqueues one launch, never waits.  A row whose user has no
    held-out item leaves its flag as it was (`flags` you pass in should start as zeros)."""

    def __init__(self, device, n_items: int, heldout_indptr, heldout_items, user_num: int, indptr=None, items=None):
        import torch
        self.lib = _lib.hip()
        self.device = torch.device(device)
        self.n_items, self.user_num = int(n_items), int(user_num)
        if not 1 <= self.n_items <= 2 ** 31 - 2 or self.user_num < 1:
            raise ValueError(f"rank_heldout: {n_items} items outside [1, 2^31 - 2] or user_num = {user_num} below 1")
        h_indptr, h_items = check_csr(heldout_indptr, heldout_items, self.user_num, self.n_items, "heldout", "held-out items")
        self.heldout = (h_indptr, h_items)
        self._h_indptr = torch.from_numpy(h_indptr).to(self.device)
        self._h_items = torch.from_numpy(h_items).to(self.device)
        self._indptr = self._items = None
        if indptr is not None:
            indptr, items = check_csr(indptr, items, self.user_num, self.n_items)
            self._indptr = torch.from_numpy(indptr).to(self.device)
            self._items = torch.from_numpy(items).to(self.device)
        self.ranks = torch.zeros(len(h_items), dtype=torch.int32, device=self.device)

    def rank(self, scores, users, flags=None):
        import torch
        n, stride = (int(scores.shape[0]), int(scores.shape[1])) if scores.dim() == 2 else (0, 0)
        if scores.dtype != torch.float32 or scores.dim() != 2 or not scores.is_contiguous() or scores.device != self.ranks.device \
                or n < 1 or stride < self.n_items:
            raise ValueError(f"rank_heldout: scores must be a contiguous fp32 device tensor [n >= 1, >= {self.n_items}]")
        if users.dtype != torch.int64 or tuple(users.shape) != (n,) or users.device != self.ranks.device or not users.is_contiguous():
            raise ValueError("rank_heldout: users must be a contiguous int64 device tensor [n]")
        if flags is None:
            flags = torch.zeros(n, dtype=torch.int32, device=self.device)
        if flags.dtype != torch.int32 or tuple(flags.shape) != (n,) or flags.device != self.ranks.device or not flags.is_contiguous():
            raise ValueError("rank_heldout: flags must be a contiguous int32 device tensor [n]")
        excl = self._indptr is not None
        _lib.check(self.lib.pmgt_rank_heldout(scores.data_ptr(), stride, n, self.n_items, users.data_ptr(),
                                              self._indptr.data_ptr() if excl else 0, self._items.data_ptr() if excl and len(self._items) else 0,
                                              self.user_num, len(self._items) if excl else 0, self._h_indptr.data_ptr(),
                                              self._h_items.data_ptr() if len(self._h_items) else 0, len(self._h_items), self.ranks.data_ptr(),
                                              flags.data_ptr(), _lib.stream()))
        return self.ranks, flags


class CatalogueMetrics:
    """pmgt_rank_heldout_reduce: owns the cut-offs, the discount tables of metrics.discount_tables on the device, the per-user records fp64
    [3 len(ks) + 1, max_users] and the 128-byte header.  reduce(ranker, users, flags) enqueues the two launches; result() and per_user()
    read the device."""

    def __init__(self, device, max_users: int, ks=(10, 20)):
        import torch
        from .metrics import check_ks, discount_tables
        self.lib = _lib.hip()
        self.device = torch.device(device)
        self.ks = check_ks(ks)
        self.max_users = int(max_users)
        if self.max_users < 1:
            raise ValueError(f"CatalogueMetrics: max_users = {max_users!r} below 1")
        self._ks_c = (C.c_int * len(self.ks))(*self.ks)
        disc, idcg = discount_tables(self.ks[-1])
        self._disc = torch.from_numpy(np.ascontiguousarray(disc)).to(self.device)
        self._idcg = torch.from_numpy(np.ascontiguousarray(idcg)).to(self.device)
        self._records = torch.zeros(3 * len(self.ks) + 1, self.max_users, dtype=torch.float64, device=self.device)
        self._header = torch.zeros(RANK_HELDOUT_HEADER_BYTES // 8, dtype=torch.float64, device=self.device)
        self._view = None
        self.n_users = 0

    def reduce(self, ranker: HeldoutRanks, users, flags=None) -> None:
        """users int64 [U <= max_users] on the device: the evaluated users; flags int32 [U] aligned with them, or None."""
        import torch
        n = int(users.shape[0])
        if users.dtype != torch.int64 or users.dim() != 1 or not 1 <= n <= self.max_users or users.device != self._header.device \
                or not users.is_contiguous():
            raise ValueError(f"CatalogueMetrics: users must be a contiguous int64 device tensor [1 .. {self.max_users}]")
        if flags is not None and (flags.dtype != torch.int32 or tuple(flags.shape) != (n,) or flags.device != self._header.device
                                  or not flags.is_contiguous()):
            raise ValueError("CatalogueMetrics: flags must be a contiguous int32 device tensor [U]")
        self._view = self._records.view(-1)[: (3 * len(self.ks) + 1) * n].view(3 * len(self.ks) + 1, n)      # the records' rows are n long
        _lib.check(self.lib.pmgt_rank_heldout_reduce(ranker.ranks.data_ptr(), ranker._h_indptr.data_ptr(), users.data_ptr(),
                                                     0 if flags is None else flags.data_ptr(), n, ranker.user_num, int(ranker.ranks.numel()),
                                                     self._ks_c, len(self.ks), self._disc.data_ptr(), self._idcg.data_ptr(),
                                                     self._view.data_ptr(), self._header.data_ptr(), _lib.stream()))
        self.n_users = n

    def statistic(self) -> dict:
        """The header: the sums per k, the rr sum and the counts (the one small device-to-host copy)."""
        if self.n_users < 1:
            raise ValueError("CatalogueMetrics: nothing was reduced")
        h = self._header.cpu().numpy()
        u = h.view(np.uint64)
        nk = RANK_MAX_KS
        return dict(ndcg={k: float(h[i]) for i, k in enumerate(self.ks)}, recall={k: float(h[nk + i]) for i, k in enumerate(self.ks)},
                    hit={k: float(h[2 * nk + i]) for i, k in enumerate(self.ks)}, rr=float(h[3 * nk]), n_users=int(u[13]), n_nan=int(u[14]),
                    n_excluded=int(u[15]))

    def per_user(self) -> dict:
        """The user records of the last reduce as numpy: ndcg[k], recall[k], hit[k], rr fp64 [U]."""
        if self.n_users < 1:
            raise ValueError("CatalogueMetrics: nothing was reduced")
        rec = self._view.cpu().numpy()
        nk = len(self.ks)
        return dict(ndcg={k: rec[i].copy() for i, k in enumerate(self.ks)}, recall={k: rec[nk + i].copy() for i, k in enumerate(self.ks)},
                    hit={k: rec[2 * nk + i].copy() for i, k in enumerate(self.ks)}, rr=rec[3 * nk].copy())


def rank_device(scorer, ids, batch: int, heldout, exclusion, id_num: int, ks, records: bool = False):
    """The ranking pass on the device: per batch of `ids` (int64 numpy, ascending, checked by the caller) scorer.score then
    HeldoutRanks.rank, with the held-out and the exclusion CSR over `id_num` ids, then one reduce.  Everything is uploaded and built
    before the first score; nothing is copied to the host and nothing waits up to statistic(), the one small copy out.
    -> (sums: CatalogueMetrics.statistic(), with n_nan; records: users, n_pos, ndcg[k], recall[k], hit[k], rr per id, or None unless
    `records`; ranks int32 aligned with the held-out CSR, or None)."""
    import torch
    dev, n, n_items = scorer.device, len(ids), scorer.n_items
    ranker = HeldoutRanks(dev, n_items, heldout[0], heldout[1], id_num, exclusion[0], exclusion[1])
    reducer = CatalogueMetrics(dev, n, ks)
    ids_d = torch.from_numpy(ids).to(dev)
    flags_d = torch.zeros(n, dtype=torch.int32, device=dev)
    work = torch.empty(batch, n_items, dtype=torch.float32, device=dev)
    for lo in range(0, n, batch):
        hi = min(lo + batch, n)
        scorer.score(ids_d[lo:hi], out=work)
        ranker.rank(work[: hi - lo], ids_d[lo:hi], flags_d[lo:hi])
    reducer.reduce(ranker, ids_d, flags_d)
    sums = reducer.statistic()                               # the one small copy out: after the loop
    if not records:
        return sums, None, None
    rec = reducer.per_user()
    rec.update(users=ids, n_pos=np.diff(heldout[0])[ids])
    return sums, rec, ranker.ranks.cpu().numpy()


def evaluate_catalogue(model, sampler, heldout, exclude=None, ks=(10, 20), batch_users: int = None, impl: str = "device", table=None,
                       threads: int = 8, seed: int = 0, per_user: bool = False):
    """Whole-catalogue ranking quality of `model` on the held-out (user, item) pairs -> {"n<k>", "r<k>", "hr<k>" for k in ks, "mrr",
    "users", "pairs"}: mean nDCG@k, Recall@k and hit rate@k, the mean reciprocal rank of each user's best held-out item, the number of
    evaluated users and of held-out pairs.  Every held-out item is ranked among ALL items of the catalogue that are not in the user's
    exclusion list, in recommend()'s order: the metrics are those of the lists recommend() returns.
    heldout, exclude: iterables of (user, item) pairs or ready (indptr, items) CSR pairs over user ids (exclude: typically the training
      interactions; None excludes nothing).  Held-out duplicates are dropped.  The evaluated users are those with at least one held-out
      item, in ascending id order.
    model, sampler, table, batch_users and the eval-mode handling are recommend()'s, for a PMGT_NCF, the stand-alone NCF class and a DCN.
    impl="device": rank_device with the class's fused scorer; the ranks are exact for the scorer's scores whatever `batch_users` is.
    impl="host": the yardstick -- rank_host over host_scores / dcn_host_scores; needs no GPU on a CPU model.
    per_user=True: returns (result, dict) with users, n_pos, ndcg[k], recall[k], hit[k], rr per evaluated user, and ranks with the
      held-out CSR (indptr, items) they align with.
    Raises ValueError for ids outside the model's tables, a held-out pair that is also excluded (naming how many), a user with a NaN score
    among their eligible items (naming how many users), an empty held-out set, and -- impl="device" only -- a head shape the kernels do
    not cover."""
    from .metrics import check_ks
    check_impl(impl)
    ks = check_ks(ks)
    user_num, n_items = model.user_num, model.item_num
    held = heldout_csr(heldout, user_num, n_items)
    exclusion, users = heldout_queries("evaluate_catalogue", held, lambda: exclusion_csr(exclude, user_num, n_items), n_items)
    dispatch = ModelDispatch(model, "evaluate_catalogue")
    if impl == "device":
        dispatch.check_covered()
    batch = check_batch(batch_users, len(users), n_items, "evaluate_catalogue")
    dispatch.resolve_table(sampler, table, threads, seed)
    with dispatch.eval_mode(impl):
        if impl == "host":
            sums, pu, ranks = rank_host(dispatch.host_scores, users, batch, held, exclusion, ks)
        else:
            import torch
            with torch.no_grad():
                sums, pu, ranks = rank_device(dispatch.scorer(), users, batch, held, exclusion, user_num, ks, per_user)
    refuse_nan("evaluate_catalogue", sums["n_nan"], len(users), "users")
    result = summarize_catalogue(sums, len(users), len(held[1]), ks)
    if not per_user:
        return result
    pu.update(ranks=ranks, indptr=held[0], items=held[1])
    return result, pu
