"""Nearest items from the embeddings: every item of the catalogue scored against a query item by the cosine (or the dot product) of their
rows in ONE table -- the encoder's CLS vectors as encode_catalogue / export_embeddings return them --, the k best per query
(similar_items) and the exact places of a query's true graph neighbours among all other items (evaluate_neighbours).  The graph-structure
objective scores a pair of nodes by exactly this cosine (pmgt/pmgt/losses.py PMGTGraphConstructLoss: F.normalize, then a dot product), so
evaluate_neighbours on held-out edges says whether pre-training worked before any head is trained; the reference has no such path.

THE SCORE (pmgt_item_sim_score, ops/item_sim.hip): dot(i, j) = the fp32 fmaf chain over k ascending; cosine = (dot * inv[min(i, j)]) *
inv[max(i, j)] with inv[j] = 1 / max(|x_j|, eps).  Symmetric bit for bit, independent of the batch, a NaN stays in its row and column.
THE ORDER is recommend()'s: descending `score_key`, among equal keys THE LOWER ITEM INDEX FIRST.  Selection, ranks and metrics are
recommend.TopkRows and catalogue_eval.HeldoutRanks / CatalogueMetrics unchanged, with the query items in the place of the users.

The pure-numpy part (item_sim_host, edges_csr, holdout_edges and impl="host") needs no GPU."""
import numpy as np

from . import _lib
from ._lib import ITEM_SIM_MAX_D, NCF_MAX_USERS, TOPK_FLAG_NAN
from .catalogue_eval import (CatalogueMetrics, HeldoutRanks, catalogue_metrics_host, count_common_pairs, heldout_queries,  # noqa: F401
                             heldout_ranks_host, rank_device, rank_host, summarize_catalogue)
from .graph import CSRGraph
from .pair_train import check_ids
from .recommend import (CatalogueScorer, TopkRows, check_batch, check_impl, check_k, default_batch_users, exclusion_csr,  # noqa: F401
                        refuse_nan, select_device, select_host, topk_host)

METRICS = ("cosine", "dot")


# ---- host side: pure numpy ------------------------------------------------------------------------------------------------------------------
def check_metric(metric) -> str:
    if metric not in METRICS:
        raise ValueError(f"metric={metric!r}: expected 'cosine' or 'dot'")
    return metric


def check_table(table, who: str):
    """ValueError in the name of `who` unless `table` is a two-dimensional fp32 numpy array or torch tensor [I >= 1, d in [1, ITEM_SIM_MAX_D]]
    -> (I, d)"""
    shape, dtype = getattr(table, "shape", None), str(getattr(table, "dtype", "")).replace("torch.", "")
    if shape is None or len(shape) != 2 or dtype != "float32" or shape[0] < 1:
        raise ValueError(f"{who}: the table must be an fp32 array or tensor [I >= 1, d]")
    if not 1 <= shape[1] <= ITEM_SIM_MAX_D:
        raise ValueError(f"{who}: d = {int(shape[1])} outside [1, {ITEM_SIM_MAX_D}]")
    if shape[0] > 2 ** 31 - 2:
        raise ValueError(f"{who}: {int(shape[0])} items outside [1, 2^31 - 2]")
    return int(shape[0]), int(shape[1])


def host_table(table) -> np.ndarray:
    """`table` as a numpy array (a torch tensor is copied to the host)"""
    if isinstance(table, np.ndarray):
        return table
    return table.detach().cpu().numpy()


def item_sim_host(table, queries=None, metric: str = "cosine", eps: float = 1e-12, dtype=np.float32) -> np.ndarray:
    """The yardstick of pmgt_item_sim_score, pure numpy in `dtype` (np.float64 for the measure): scores [n, I] of the items `queries`
    (None: every item, in order) against every row of `table` [I, d].  metric "dot": the product of the rows; "cosine":
    (dot * inv[min(i, j)]) * inv[max(i, j)] with inv[j] = 1 / max(sqrt(sum_k x_jk^2), eps), the kernel's order of the two scalings.  The
    sums are numpy's (no fmaf chain)."""
    check_metric(metric)
    t = np.ascontiguousarray(host_table(table), dtype=dtype)
    if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"item_sim_host: table {t.shape} must be [I >= 1, d >= 1]")
    n_items = t.shape[0]
    q = np.arange(n_items, dtype=np.int64) if queries is None else np.ascontiguousarray(queries, dtype=np.int64)
    if q.ndim != 1:
        raise ValueError(f"item_sim_host: queries {q.shape} must be one-dimensional")
    check_ids("queries", q, n_items, "item_sim_host")
    dot = t[q] @ t.T
    if metric == "dot":
        return dot
    with np.errstate(invalid="ignore"):
        inv = (1 / np.maximum(np.sqrt((t * t).sum(axis=1)), dtype(eps))).astype(dtype)
    j = np.arange(n_items, dtype=np.int64)
    lo, hi = np.minimum(q[:, None], j[None, :]), np.maximum(q[:, None], j[None, :])
    return (dot * inv[lo]) * inv[hi]


def edges_csr(edges, n_items: int, symmetric: bool = True, who: str = "edges"):
    """The CSR over item ids of a set of edges given as (item, item) index pairs: every edge (a, b) puts b into the list of a and, with
    `symmetric`, a into the list of b.  -> (indptr int64 [n_items + 1], items int32), every list sorted with DUPLICATES DROPPED."""
    pairs = np.asarray(edges if isinstance(edges, np.ndarray) else list(edges if edges is not None else ()))
    if pairs.size == 0:
        return np.zeros(n_items + 1, dtype=np.int64), np.zeros(0, dtype=np.int32)
    if pairs.ndim != 2 or pairs.shape[1] != 2 or not np.issubdtype(pairs.dtype, np.integer):
        raise ValueError(f"{who}: expected (item, item) integer pairs, got an array of shape {pairs.shape} and dtype {pairs.dtype}")
    pairs = pairs.astype(np.int64)
    check_ids("items", pairs, n_items, who)
    if symmetric:
        pairs = np.concatenate([pairs, pairs[:, ::-1]])
    key = np.unique(pairs[:, 0] * np.int64(n_items) + pairs[:, 1])
    indptr = np.zeros(n_items + 1, dtype=np.int64)
    np.cumsum(np.bincount(key // n_items, minlength=n_items), out=indptr[1:])
    return indptr, (key % n_items).astype(np.int32)


def graph_pairs(graph: CSRGraph, n_items: int, who: str) -> np.ndarray:
    """The directed (row, row) pairs of a CSRGraph over the catalogue: node id v is row v - 2"""
    if graph.n_nodes != n_items:
        raise ValueError(f"{who}: the graph has {graph.n_nodes} nodes, the table {n_items} rows")
    owner = np.repeat(np.arange(n_items, dtype=np.int64), np.diff(graph.indptr)[2:])
    return np.stack([owner, graph.indices[graph.indptr[2]:] - 2], axis=1)


def item_exclusion_csr(exclude, n_items: int, exclude_self: bool, who: str = "exclude"):
    """exclusion_csr over item ids -- `exclude` None, (query, item) pairs, a ready (indptr, items) pair or a CSRGraph over the catalogue --
    plus, with `exclude_self`, (i, i) for every item; every list sorted, duplicates dropped."""
    if isinstance(exclude, CSRGraph):
        exclude = graph_pairs(exclude, n_items, who)
    indptr, items = exclusion_csr(exclude, n_items, n_items, who)
    if not exclude_self:
        return indptr, items
    owner = np.repeat(np.arange(n_items, dtype=np.int64), np.diff(indptr))
    own = np.arange(n_items, dtype=np.int64)
    return edges_csr(np.stack([np.concatenate([owner, own]), np.concatenate([items.astype(np.int64), own])], axis=1), n_items, False, who)


def holdout_edges(graph: CSRGraph, fraction: float = 0.1, seed: int = 0):
    """Split the undirected edges of `graph` for evaluate_neighbours -> (train CSRGraph, heldout int64 [H, 2] item rows (node id - 2) with
    a < b).  A pure function of its arguments: the undirected edges (in adjacency order of their lower end) are permuted by
    np.random.default_rng(seed) and walked once in that order; an edge is held out only while BOTH endpoints keep at least one other
    remaining edge, until round(fraction * E) edges are out or the list ends.  The train graph keeps every node (validate() passes: the
    reference's sampling is undefined for isolated nodes), the remaining edges in their original adjacency order with their weights."""
    if not isinstance(graph, CSRGraph):
        raise ValueError("holdout_edges: expected a CSRGraph (an ItemGraph's .graph serves)")
    if not (isinstance(fraction, (int, float, np.floating)) and 0.0 <= float(fraction) < 1.0):
        raise ValueError(f"holdout_edges: fraction = {fraction!r} outside [0, 1)")
    n = graph.n_nodes
    deg = np.diff(graph.indptr)
    src = np.repeat(np.arange(n + 2, dtype=np.int64), deg)
    dst = graph.indices
    fwd = src < dst
    edges = np.stack([src[fwd], dst[fwd]], axis=1)
    if 2 * len(edges) != len(dst):
        raise ValueError("holdout_edges: the graph is not symmetric or has self edges")
    target = int(round(float(fraction) * len(edges)))
    left = deg.copy()
    out = []
    for e in np.random.default_rng(seed).permutation(len(edges)):
        if len(out) >= target:
            break
        a, b = edges[e]
        if left[a] > 1 and left[b] > 1:
            left[a] -= 1
            left[b] -= 1
            out.append(e)
    held = edges[np.asarray(out, dtype=np.int64)].reshape(-1, 2)
    key = np.minimum(src, dst) * np.int64(n + 2) + np.maximum(src, dst)
    keep = ~np.isin(key, held[:, 0] * np.int64(n + 2) + held[:, 1])
    indptr = np.zeros(n + 3, dtype=np.int64)
    np.cumsum(np.bincount(src[keep], minlength=n + 2), out=indptr[1:])
    return CSRGraph(n, indptr, dst[keep], graph.weights[keep]), held - 2


# ---- device side ------------------------------------------------------------------------------------------------------------------------------
def device_table(table, who: str):
    """`table` as a contiguous fp32 device tensor: a device tensor as it is, a numpy array uploaded once"""
    import torch
    if isinstance(table, np.ndarray):
        if not torch.cuda.is_available():
            raise ValueError(f"{who}: impl='device' needs a GPU")
        return torch.from_numpy(np.ascontiguousarray(table)).cuda()
    if not isinstance(table, torch.Tensor) or not table.is_cuda:
        raise ValueError(f"{who}: the table must be a numpy array or an fp32 tensor on a GPU")
    return table.detach().contiguous()


class ItemSimScorer(CatalogueScorer):
    """pmgt_item_sim_score over one table [I, d] (fp32, contiguous, on a GPU), read in place: ItemSimScorer(table) computes the inverse norms
    once (pmgt_item_sim_norms; metric "dot" has none); score(queries) launches.  Nothing in here copies to the host or waits for the device."""
    entry, ids_name, max_ids = "item_sim", "queries", NCF_MAX_USERS

    def __init__(self, table, metric: str = "cosine", eps: float = 1e-12):
        import torch
        self.metric = check_metric(metric)
        self.n_items, self.d = check_table(table, "item_sim")
        if not isinstance(table, torch.Tensor) or not table.is_cuda or not table.is_contiguous():
            raise ValueError("item_sim: the table must be a contiguous fp32 tensor on a GPU")
        eps = float(np.float32(eps))
        if not (np.isfinite(eps) and eps > 0.0):
            raise ValueError(f"item_sim: eps = {eps!r} is not a positive finite number")
        self.lib = _lib.hip()
        self.table = table.detach()
        self.device = table.device
        self.inv_norm = None
        if metric == "cosine":
            self.inv_norm = torch.empty(self.n_items, dtype=torch.float32, device=self.device)
            with torch.cuda.device(self.device):
                _lib.check(self.lib.pmgt_item_sim_norms(self.table.data_ptr(), self.n_items, self.d, eps, self.inv_norm.data_ptr(), _lib.stream()))

    def _launch(self, queries, n, out):
        _lib.check(self.lib.pmgt_item_sim_score(self.table.data_ptr(), 0 if self.inv_norm is None else self.inv_norm.data_ptr(), queries.data_ptr(),
                                                n, self.n_items, self.d, out.data_ptr(), int(out.shape[1]), _lib.stream()))


def similar_items(table, items=None, k: int = 20, metric: str = "cosine", exclude=None, exclude_self: bool = True, batch_items: int = None,
                  impl: str = "device"):
    """For every item of `items` (None: every item of the table, in order), the k items of the whole catalogue most similar to it by
    `metric` ("cosine" or "dot") that are not in its exclusion list -> (neighbours int64 [Q, k], scores fp32 [Q, k]) as numpy, best first;
    ties rank the lower item index first.
    table: [I, d] fp32 -- the device tensor encode_catalogue returns, or a numpy array such as export_embeddings returns (impl="device"
      uploads it once); read in place, never normalised.
    exclude: an iterable of (query item, item) pairs, a ready (indptr, items) CSR pair over item ids, or a CSRGraph over the catalogue (node
      id v = row v - 2); built into the CSR once.  exclude_self adds (i, i) for every item.
    A query with FEWER THAN k eligible items gets item -1 and score -inf in the slots past them; that is not an error.
    batch_items: queries per launch; None picks the largest batch whose [batch, I] fp32 score rows stay within 256 MiB.
    impl="device": recommend.select_device with an ItemSimScorer.  impl="host": the yardstick -- select_host over item_sim_host; needs no GPU.
    Raises ValueError for ids outside the table, k outside [1, 1024], d outside [1, 1024], an unknown metric or impl, and a query with a
    NaN score among its eligible items (naming how many)."""
    check_impl(impl)
    check_metric(metric)
    k = check_k(k)
    n_items, _ = check_table(table, "similar_items")
    items = np.arange(n_items, dtype=np.int64) if items is None else np.ascontiguousarray(items, dtype=np.int64)
    if items.ndim != 1 or len(items) < 1:
        raise ValueError(f"similar_items: items {items.shape} must be [Q >= 1]")
    check_ids("items", items, n_items, "similar_items")
    indptr, excl = item_exclusion_csr(exclude, n_items, exclude_self)
    batch = check_batch(batch_items, len(items), n_items, "similar_items", "batch_items")
    if impl == "host":
        t = host_table(table)
        found, scores, flags = select_host(lambda q: item_sim_host(t, q, metric), items, batch, k, indptr, excl)
    else:
        import torch
        table_d = device_table(table, "similar_items")
        with torch.no_grad(), torch.cuda.device(table_d.device):
            found, scores, flags = select_device(ItemSimScorer(table_d, metric), items, batch, k, indptr, excl, n_items)
    refuse_nan("similar_items", int(np.count_nonzero(flags & TOPK_FLAG_NAN)), len(items), "items")
    return found.astype(np.int64), scores


def evaluate_neighbours(table, heldout, exclude=None, ks=(10, 20), metric: str = "cosine", exclude_self: bool = True, batch_items: int = None,
                        impl: str = "device", per_item: bool = False):
    """Whole-catalogue quality of the embeddings `table` [I, d] on held-out graph edges -> {"n<k>", "r<k>", "hr<k>" for k in ks, "mrr",
    "items", "pairs"}: evaluate_catalogue's dictionary with the query items in the place of the users.  Every item with a held-out
    neighbour ranks ALL other items of the catalogue by `metric` with its own row, in similar_items' order, and the metrics say where its
    held-out neighbours land: mean nDCG@k, Recall@k, hit rate@k and the mean reciprocal rank of the best one.
    heldout: undirected edges as (item, item) index pairs (holdout_edges' second result): every edge (a, b) makes b a held-out item of
      query a and a a held-out item of query b; duplicates are dropped.  The evaluated items are those with at least one, ascending.
    exclude: typically the training graph -- a CSRGraph (node id v = row v - 2), (query item, item) pairs or a ready (indptr, items) CSR pair
      over item ids; None excludes nothing.  exclude_self adds (i, i) for every item.
    table, metric, batch_items, impl: similar_items'.  impl="device": catalogue_eval.rank_device with an ItemSimScorer.  impl="host": the
      yardstick -- rank_host over item_sim_host; needs no GPU.
    per_item=True: returns (result, dict) with items (the evaluated queries), n_pos, ndcg[k], recall[k], hit[k], rr per evaluated item, and
      ranks with the held-out CSR (indptr, heldout) they align with.
    Raises ValueError for ids outside the table, a held-out pair that is also excluded (naming how many), a query with a NaN score among
    its eligible items (naming how many), an empty held-out set, d outside [1, 1024] and an unknown metric or impl."""
    from .metrics import check_ks
    check_impl(impl)
    check_metric(metric)
    ks = check_ks(ks)
    n_items, _ = check_table(table, "evaluate_neighbours")
    held = edges_csr(heldout, n_items, True, "heldout")
    exclusion, items = heldout_queries("evaluate_neighbours", held, lambda: item_exclusion_csr(exclude, n_items, exclude_self), n_items)
    batch = check_batch(batch_items, len(items), n_items, "evaluate_neighbours", "batch_items")
    if impl == "host":
        t = host_table(table)
        sums, rec, ranks = rank_host(lambda q: item_sim_host(t, q, metric), items, batch, held, exclusion, ks)
    else:
        import torch
        table_d = device_table(table, "evaluate_neighbours")
        with torch.no_grad(), torch.cuda.device(table_d.device):
            sums, rec, ranks = rank_device(ItemSimScorer(table_d, metric), items, batch, held, exclusion, n_items, ks, per_item)
    refuse_nan("evaluate_neighbours", sums["n_nan"], len(items), "items")
    result = summarize_catalogue(sums, len(items), len(held[1]), ks)
    result = {("items" if key == "users" else key): v for key, v in result.items()}
    if not per_item:
        return result
    rec.pop("users")
    rec.update(items=items, ranks=ranks, indptr=held[0], heldout=held[1])
    return result, rec
