"""The item graph from (user, item) interactions: the reference's "Construct Product Graph" cell (notebooks/PMGT.ipynb, cell 20), the one
stage in front of graph.gpickle.  With A the BINARY item-by-user matrix, C = A A^T counts the users two items share; an edge joins i != j
with C[i, j] >= min_count (the reference: 3); the nodes are the items that keep at least one edge, numbered 2 .. N + 1 in ascending
catalogue index (the `classes_` of the reference's node_encoder); the weight of an edge is
      (ln c + 1) / (ln sqrt(deg_i deg_j) + 1),      c = C[i, j],  deg = the number of kept edges of the item.

NEIGHBOUR ORDER is part of the sampler's contract (graph.py) and the reference fixes none: its rows are filled from Python sets of
reviewer-id strings, so two runs of the notebook order the same adjacency lists differently.  The builder therefore defines it: A NODE'S
NEIGHBOURS IN ASCENDING NODE ID, which is what CSRGraph.from_edge_list gives for the edge list (i < j) sorted row-major.  What the
reference does fix -- node set, edge set, count and weight of every edge -- is reproduced exactly, the weights bit for bit: everything up
to the weight is integer arithmetic, and the weights are one numpy expression over the integer counts and degrees on both paths.

item_graph_host is the numpy yardstick (no GPU, no scipy); build_item_graph(impl="device") counts on the device (ops/item_graph.hip)."""
from __future__ import annotations

import numpy as np

from .graph import CSRGraph

MAX_ITEMS = 2 ** 31 - 2       # item indices and node ids fit an int32
MAX_USER = 2 ** 31            # user ids lie below it: user * num_item + item fits an int64
MAX_PAIRS = 2 ** 31 - 1       # distinct pairs
DENSE_MAX_ITEMS = 2048        # item_graph_host: a dense count matrix up to this many items ...
DENSE_MAX_CELLS = 1 << 24     # ... and this many cells of the item-by-user matrix (fp64: 128 MiB); the sorted-key form above either
HOST_CHUNK = 1 << 24          # expansions one step of the sorted-key form holds
SCRATCH_BYTES = 1 << 30       # the pool of dense fallback rows is bounded by this


class ItemGraph:
    """What build_item_graph returns.
    graph          CSRGraph, node ids 2 .. N + 1, every adjacency list strictly ascending; validate() passes by construction
    items          int64 [N]: the catalogue index of node n + 2, ascending
    node_of_item   int64 [num_item]: the node id of an item, or -1
    counts         int64, aligned with graph.indices: the co-review count of each stored neighbour
    fallback_items int64: the catalogue indices of the rows the device counted in a dense scratch row (empty for impl="host")"""

    def __init__(self, graph: CSRGraph, items, node_of_item, counts, fallback_items=None):
        self.graph = graph
        self.items = np.ascontiguousarray(items, dtype=np.int64)
        self.node_of_item = np.ascontiguousarray(node_of_item, dtype=np.int64)
        self.counts = np.ascontiguousarray(counts, dtype=np.int64)
        self.fallback_items = np.zeros(0, dtype=np.int64) if fallback_items is None else np.ascontiguousarray(fallback_items, dtype=np.int64)

    def filter_pairs(self, pairs):
        """The rows of `pairs` ([P, 2] of (user, item), numpy or torch) whose item is a node (notebook cell 24), in their order."""
        item = pairs[:, 1]
        if isinstance(pairs, np.ndarray):
            inside = (item >= 0) & (item < len(self.node_of_item))
            keep = inside & (self.node_of_item[np.where(inside, item, 0)] >= 0)
            return pairs[keep]
        import torch
        table = torch.from_numpy(self.node_of_item).to(pairs.device)
        inside = (item >= 0) & (item < len(self.node_of_item))
        keep = inside & (table[torch.where(inside, item, torch.zeros_like(item))] >= 0)
        return pairs[keep]

    def to_networkx(self):
        """nx.Graph over CATALOGUE indices with a float `weight` per edge: the graph to hand back to the reference."""
        import networkx as nx
        g = self.graph
        row = np.repeat(np.arange(g.n_nodes + 2, dtype=np.int64), np.diff(g.indptr))
        upper = row < g.indices
        out = nx.Graph()
        out.add_weighted_edges_from(zip(self.items[row[upper] - 2].tolist(), self.items[g.indices[upper] - 2].tolist(),
                                        g.weights[upper].tolist()))
        return out


def edge_weights(counts, deg_a, deg_b):
    """(ln c + 1) / (ln sqrt(deg_a deg_b) + 1) in fp64 from integer arrays: the one expression both paths use."""
    c = np.asarray(counts, dtype=np.int64)
    prod = np.asarray(deg_a, dtype=np.int64) * np.asarray(deg_b, dtype=np.int64)
    return (np.log(c) + 1) / (np.log(np.sqrt(prod)) + 1)


def synthetic_interactions(num_user: int, num_item: int, n_pairs: int, seed: int = 0, item_exponent: float = 0.7,
                           user_exponent: float = 0.5) -> np.ndarray:
    """Seeded interaction set int64 [n_pairs, 2] of (user, item) with Zipf-like marginals: the r-th most popular item (most active user) is
    drawn with probability proportional to (r + 1)^-exponent, the ranks dealt to the ids by a seeded permutation; users and items are drawn
    independently, so rows repeat (duplicates count once in the graph)."""
    rs = np.random.RandomState(seed)
    cols = []
    for n, a in ((num_user, user_exponent), (num_item, item_exponent)):
        p = (np.arange(n, dtype=np.float64) + 1.0) ** -float(a)
        cdf = np.cumsum(p / p.sum())
        rank = np.minimum(np.searchsorted(cdf, rs.random_sample(n_pairs), side="right"), n - 1)
        cols.append(rs.permutation(n).astype(np.int64)[rank])
    return np.stack(cols, 1)


# ---- checks -----------------------------------------------------------------------------------------------------------------------------------
def _is_torch(x) -> bool:
    return type(x).__module__.split(".")[0] == "torch"


def _check_arguments(pairs, num_item, min_count):
    if isinstance(num_item, bool) or not isinstance(num_item, (int, np.integer)) or num_item < 1:
        raise ValueError(f"item graph: num_item = {num_item!r} must be a positive integer")
    if num_item > MAX_ITEMS:
        raise ValueError(f"item graph: num_item = {num_item} above 2^31 - 2")
    if isinstance(min_count, bool) or not isinstance(min_count, (int, np.integer)) or min_count < 1:
        raise ValueError(f"item graph: min_count = {min_count!r} must be an integer >= 1")
    if _is_torch(pairs):
        import torch
        ok = pairs.dtype == torch.int64 and pairs.dim() == 2 and pairs.shape[1] == 2
    else:
        ok = isinstance(pairs, np.ndarray) and pairs.dtype == np.int64 and pairs.ndim == 2 and pairs.shape[1] == 2
    if not ok:
        raise ValueError("item graph: pairs must be an int64 array or tensor [P, 2] of (user, item)")


def _check_ranges(lo_user, hi_user, lo_item, hi_item, num_item):
    if lo_user < 0 or lo_item < 0:
        raise ValueError("item graph: negative id in pairs")
    if hi_item >= num_item:
        raise ValueError(f"item graph: item {hi_item} outside [0, num_item = {num_item})")
    if hi_user >= MAX_USER:
        raise ValueError(f"item graph: user id {hi_user} is not below 2^31")


def _no_edge(min_count, largest):
    return ValueError(f"item graph: no pair of items is co-reviewed by min_count = {min_count} users (the largest count seen is {largest}): "
                      f"the graph has no edge")


# ---- host ---------------------------------------------------------------------------------------------------------------------------------------
def _host_pairs(pairs, num_item):
    """-> the sorted distinct keys user * num_item + item of validated pairs (numpy int64)"""
    p = pairs.detach().cpu().numpy() if _is_torch(pairs) else pairs
    if len(p):
        _check_ranges(int(p[:, 0].min()), int(p[:, 0].max()), int(p[:, 1].min()), int(p[:, 1].max()), num_item)
    keys = np.unique(p[:, 0] * np.int64(num_item) + p[:, 1])
    if len(keys) > MAX_PAIRS:
        raise ValueError(f"item graph: {len(keys)} distinct pairs, more than 2^31 - 1")
    return keys


def _upper_counts_dense(user, item, num_item, n_users):
    a = np.zeros((num_item, n_users), dtype=np.float64)      # small integers in fp64: the product is exact
    a[item, user] = 1.0
    c = np.rint(a @ a.T).astype(np.int64)
    i, j = np.nonzero(np.triu(c, 1))                         # row-major, i < j
    return i.astype(np.int64), j.astype(np.int64), c[i, j]


def _upper_counts_sorted(item, user_ptr, num_item):
    """Every user's item pairs (a < b) as keys a * num_item + b, counted: steps of at most HOST_CHUNK expansions, merged by key."""
    after = np.repeat(user_ptr[1:], np.diff(user_ptr)) - np.arange(len(item), dtype=np.int64) - 1      # partners behind each place
    ends = np.cumsum(after)
    keys, cnts = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    lo = 0
    while lo < len(item):
        start = ends[lo] - after[lo]
        hi = max(lo + 1, int(np.searchsorted(ends, start + HOST_CHUNK, side="right")))
        n = after[lo:hi]
        src = np.repeat(np.arange(lo, hi, dtype=np.int64), n)
        dst = src + 1 + (np.arange(len(src), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n))
        k, c = np.unique(item[src] * np.int64(num_item) + item[dst], return_counts=True)
        keys, cnts = np.concatenate([keys, k]), np.concatenate([cnts, c.astype(np.int64)])
        if len(keys) > 4 * HOST_CHUNK or hi >= len(item):
            keys, inv = np.unique(keys, return_inverse=True)
            cnts = np.bincount(inv, weights=None if not len(cnts) else cnts, minlength=len(keys)).astype(np.int64)
        lo = hi
    return keys // num_item, keys % num_item, cnts


def _assemble(i, j, c, num_item, min_count, largest):
    """From the upper triangle (i < j, row-major) with counts: threshold, nodes, weights, CSR -> ItemGraph parts"""
    keep = c >= min_count
    i, j, c = i[keep], j[keep], c[keep]
    if len(c) == 0:
        raise _no_edge(min_count, largest)
    deg = np.bincount(np.concatenate([i, j]), minlength=num_item).astype(np.int64)
    items = np.nonzero(deg)[0].astype(np.int64)
    node_of_item = np.full(num_item, -1, dtype=np.int64)
    node_of_item[items] = np.arange(2, len(items) + 2, dtype=np.int64)
    edges = np.stack([node_of_item[i], node_of_item[j]], 1)
    graph = CSRGraph.from_edge_list(len(items), edges, edge_weights(c, deg[i], deg[j]))
    order = np.argsort(edges.ravel(), kind="stable")         # from_edge_list's arrangement, for the counts
    return graph, items, node_of_item, np.repeat(c, 2)[order]


def item_graph_host(pairs, num_item: int, min_count: int = 3) -> ItemGraph:
    """The yardstick, pure numpy: dedupe, count, threshold, upper triangle row-major, CSRGraph.from_edge_list.  Up to DENSE_MAX_ITEMS items
    (and DENSE_MAX_CELLS cells of the item-by-user matrix) the counts are one dense product; above, every user's item pairs are listed as
    sorted keys and counted.  Same arguments and refusals as build_item_graph."""
    _check_arguments(pairs, num_item, min_count)
    keys = _host_pairs(pairs, int(num_item))
    num_item, min_count = int(num_item), int(min_count)
    if len(keys) == 0:
        raise _no_edge(min_count, 0)
    users, user = np.unique(keys // num_item, return_inverse=True)      # compact user indices; keys are user-major, items ascending
    item = keys % num_item
    if num_item <= DENSE_MAX_ITEMS and num_item * len(users) <= DENSE_MAX_CELLS:
        i, j, c = _upper_counts_dense(user, item, num_item, len(users))
    else:
        user_ptr = np.zeros(len(users) + 1, dtype=np.int64)
        np.cumsum(np.bincount(user, minlength=len(users)), out=user_ptr[1:])
        i, j, c = _upper_counts_sorted(item, user_ptr, num_item)
    return ItemGraph(*_assemble(i, j, c, num_item, min_count, int(c.max()) if len(c) else 0))


# ---- device -------------------------------------------------------------------------------------------------------------------------------------
def device_csrs(keys, num_item: int):
    """The two CSR images of the sorted distinct keys (device int64) and the expansion length of every item row, torch ops on the device.
    -> dict: item_ptr int64 [num_item + 1], item_users int32 [P], user_ptr int64 [U + 1], user_items int32 [P], work int64 [num_item],
    n_users"""
    import torch
    user, item = keys // num_item, keys % num_item
    _, inv, per_user = torch.unique_consecutive(user, return_inverse=True, return_counts=True)
    n_users = int(per_user.numel())
    user_ptr = torch.zeros(n_users + 1, dtype=torch.int64, device=keys.device)
    torch.cumsum(per_user, 0, out=user_ptr[1:])
    by_item = torch.sort(item * n_users + inv).values        # item-major: the users of an item, as compact indices
    item_users = by_item % n_users
    item_ptr = torch.zeros(num_item + 1, dtype=torch.int64, device=keys.device)
    torch.cumsum(torch.bincount(item, minlength=num_item), 0, out=item_ptr[1:])
    run = torch.zeros(len(keys) + 1, dtype=torch.int64, device=keys.device)
    torch.cumsum(per_user[item_users], 0, out=run[1:])
    work = run[item_ptr[1:]] - run[item_ptr[:-1]]
    return dict(item_ptr=item_ptr, item_users=item_users.to(torch.int32), user_ptr=user_ptr, user_items=item.to(torch.int32),
                work=work.contiguous(), n_users=n_users)


class ItemGraphKernels:
    """pmgt_item_graph_count / pmgt_item_graph_fill over one set of CSRs: owns the degree words, the largest-count word and the zeroed
    pool of dense fallback rows.  count() and fill() enqueue two launches each and never wait."""

    def __init__(self, csrs: dict, num_item: int, min_count: int, slots: int = None):
        import torch
        from . import _lib
        self.lib = _lib.hip()
        self.slots = int(self.lib.pmgt_item_graph_default_slots() if slots is None else slots)
        if not _lib.ITEM_GRAPH_MIN_SLOTS <= self.slots <= _lib.ITEM_GRAPH_MAX_SLOTS or self.slots & (self.slots - 1):
            raise ValueError(f"item graph: slots = {slots!r} is no power of two in [{_lib.ITEM_GRAPH_MIN_SLOTS}, {_lib.ITEM_GRAPH_MAX_SLOTS}]")
        self.c, self.num_item, self.min_count = csrs, int(num_item), int(min_count)
        dev = csrs["item_ptr"].device
        self.n_pairs = int(csrs["user_items"].numel())
        stride = (self.num_item + 3) // 4 * 4
        self.scratch_rows = int(min(max(SCRATCH_BYTES // (4 * stride), 1), 1024))
        self.scratch = torch.zeros(self.scratch_rows * stride, dtype=torch.int32, device=dev)
        self.deg_flags = torch.zeros(self.num_item, dtype=torch.int32, device=dev)
        self.max_count = torch.zeros(1, dtype=torch.int32, device=dev)

    def _front(self):
        c = self.c
        return (c["item_ptr"].data_ptr(), c["item_users"].data_ptr(), c["user_ptr"].data_ptr(), c["user_items"].data_ptr(), c["work"].data_ptr(),
                self.num_item, c["n_users"], self.n_pairs, self.min_count, self.slots)

    def count(self):
        from . import _lib
        self.max_count.zero_()
        _lib.check(self.lib.pmgt_item_graph_count(*self._front(), self.deg_flags.data_ptr(), self.max_count.data_ptr(), self.scratch.data_ptr(),
                                                  self.scratch_rows, _lib.stream()))
        return self.deg_flags

    def fill(self, row_ptr, node_of_item, total: int, indices, counts):
        from . import _lib
        _lib.check(self.lib.pmgt_item_graph_fill(*self._front(), self.deg_flags.data_ptr(), row_ptr.data_ptr(), node_of_item.data_ptr(), int(total),
                                                 indices.data_ptr(), counts.data_ptr(), self.scratch.data_ptr(), self.scratch_rows, _lib.stream()))


def _item_graph_device(pairs, num_item, min_count, device, slots):
    import torch
    if _is_torch(pairs) and pairs.is_cuda:
        dev = pairs.device if device is None else torch.device(device)
        if len(pairs):      # validated where they are: one 32-byte copy of the four extremes before anything is launched
            lo, hi = pairs.min(0).values, pairs.max(0).values
            ext = torch.stack([lo, hi]).cpu().numpy()
            _check_ranges(int(ext[0, 0]), int(ext[1, 0]), int(ext[0, 1]), int(ext[1, 1]), num_item)
        p = pairs.to(dev)
    else:
        dev = torch.device("cuda" if device is None else device)
        p = pairs.detach().numpy() if _is_torch(pairs) else pairs
        if len(p):          # host pairs are validated in numpy and cost no copy back
            _check_ranges(int(p[:, 0].min()), int(p[:, 0].max()), int(p[:, 1].min()), int(p[:, 1].max()), num_item)
        p = torch.from_numpy(np.ascontiguousarray(p)).to(dev)
    if dev.type != "cuda":
        raise ValueError(f"item graph: impl='device' needs a GPU device, not {dev}")
    if len(p) == 0:
        raise _no_edge(min_count, 0)
    with torch.cuda.device(dev):
        keys = torch.unique(p[:, 0] * num_item + p[:, 1])       # sorted: user-major, items ascending; duplicates count once
        if keys.numel() > MAX_PAIRS:
            raise ValueError(f"item graph: {keys.numel()} distinct pairs, more than 2^31 - 1")
        k = ItemGraphKernels(device_csrs(keys, num_item), num_item, min_count, slots)
        deg = k.count() & 0x7FFFFFFF
        row_ptr = torch.zeros(num_item + 1, dtype=torch.int64, device=dev)
        torch.cumsum(deg, 0, dtype=torch.int64, out=row_ptr[1:])
        total = int(row_ptr[-1].item())                          # the 8-byte copy that sizes the output
        if total == 0:
            raise _no_edge(min_count, int(k.max_count.item()))   # (the error path alone reads the largest count)
        is_node = deg > 0
        node_of_item = torch.where(is_node, torch.cumsum(is_node, 0) + 1, -1).to(torch.int32)
        out = torch.empty(num_item + 2 * total, dtype=torch.int32, device=dev)      # [deg | flag << 31, indices, counts]: one copy back
        k.fill(row_ptr, node_of_item, total, out[num_item: num_item + total], out[num_item + total:])
        out[:num_item] = k.deg_flags
        host = out.cpu().numpy()
    words = host[:num_item].view(np.uint32)
    deg = (words & np.uint32(0x7FFFFFFF)).astype(np.int64)
    items = np.nonzero(deg)[0].astype(np.int64)
    n = len(items)
    node_of_item = np.full(num_item, -1, dtype=np.int64)
    node_of_item[items] = np.arange(2, n + 2, dtype=np.int64)
    indptr = np.zeros(n + 3, dtype=np.int64)
    np.cumsum(deg[items], out=indptr[3:])
    indices = host[num_item: num_item + total].astype(np.int64)
    counts = host[num_item + total:].astype(np.int64)
    node_deg = deg[items]
    row = np.repeat(np.arange(n, dtype=np.int64), node_deg)
    graph = CSRGraph(n, indptr, indices, edge_weights(counts, node_deg[row], node_deg[indices - 2]))      # (an integer product: no order in it)
    return ItemGraph(graph, items, node_of_item, counts, np.nonzero(words >> np.uint32(31))[0])


def build_item_graph(pairs, num_item: int, min_count: int = 3, impl: str = "device", device=None, slots: int = None) -> ItemGraph:
    """The item graph of a set of interactions.
    pairs      int64 [P, 2] of (user, item), numpy or torch, on the host or the device; duplicates count once and the order of the rows
               does not matter: the same set of pairs gives the same bits
    num_item   the size of the catalogue: items are indices in [0, num_item)
    min_count  an edge needs this many common users (the reference: 3)
    impl       "device": counting and thresholding in HIP (ops/item_graph.hip), the CSR images of the pairs, the scans and the numbering of the
               nodes in torch ops on the device; one 8-byte copy sizes the output between the two passes, one copy brings the degrees,
               neighbours and counts back, and the weights are computed in numpy from those integers.  "host": item_graph_host.
    slots      the entries of one wave's LDS table (a power of two, 16 .. 1024; None: the library's default).  A row with more than
               3 * slots distinct neighbours is counted in a dense scratch row instead: the result does not depend on it.
    Raises ValueError before anything is launched for pairs of another shape or dtype, a negative id, an item >= num_item,
    num_item > 2^31 - 2, a user id >= 2^31, more than 2^31 - 1 distinct pairs, min_count < 1; and for a result without any edge, naming the
    largest count seen."""
    if impl not in ("host", "device"):
        raise ValueError(f"impl={impl!r}: expected 'host' or 'device'")
    if impl == "host":
        return item_graph_host(pairs, num_item, min_count)
    _check_arguments(pairs, num_item, min_count)
    return _item_graph_device(pairs, int(num_item), int(min_count), device, slots)
