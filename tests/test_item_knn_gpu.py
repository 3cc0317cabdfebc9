"""pmgt_knn_score against its numpy yardstick over THE SAME index arrays (built on the device, copied out), compared with == and no
tolerance: the score is a fixed sequence of rounded fp32 operations.  Then the tile edges, what the definition buys (independent of the
batch, repeatable, the prefix property), the cross-check against pmgt_history_score, recommend_item_knn / evaluate_item_knn on both impls
and the refusals of the C entry."""
import functools

import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.history import HistoryScorer
from pmgt_amd.item_knn import (ItemKnnIndex, ItemKnnScorer, build_item_knn, evaluate_item_knn, item_knn_scores_host, recommend_item_knn,
                               weighted_history_csr)
from tests import item_sim_util as U

pytestmark = pytest.mark.gpu

SENTINEL = 7777.0
N_ITEMS, D = 300, 33
MS = (1, 5, 63, 64, 65, 130, 299, 400)                       # a step of the kernel is 64 slots; 400 > I - 1: padded rows
# the history lengths of users 0 .. 19; user 20 has no history, user 21 four items; USER_NUM itself is an id outside the CSR
LENGTHS = (1, 2, 31, 64, 65, 300, 5, 3, 300, 1, 64, 2, 31, 65, 7, 1, 20, 300, 2, 10)
EMPTY, SHORT, USER_NUM = 20, 21, 22
BATCHES = (1, 17, 22)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def histories():
    """the history CSR over USER_NUM users with one weight per entry; read-only"""
    rng = np.random.default_rng(11)
    lists = [np.sort(rng.choice(N_ITEMS, size=n, replace=False)) for n in LENGTHS + (0, 4)]
    indptr = np.zeros(USER_NUM + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=indptr[1:])
    items = np.concatenate(lists).astype(np.int32)
    csr, w = weighted_history_csr((indptr, items), rng.uniform(-1.0, 5.0, size=len(items)), N_ITEMS)
    for a in (csr[0], csr[1], w):
        a.setflags(write=False)
    return csr, w


@functools.lru_cache(maxsize=None)
def indexes():
    """the index at the largest m built ON THE DEVICE, and its copy on the host: the yardstick reads the kernel's own index arrays"""
    index = build_item_knn(dev(U.normal_table(D, 29)), MS[-1], batch_items=77)
    assert index.on_device and index.nbr.dtype == torch.int32 and index.sim.dtype == torch.float32 and index.nbr.is_contiguous()
    return index, index.host()


def fused(scorer, users, slack=0):
    """the kernel's rows [len(users), I]; with `slack`, into a wider buffer whose columns past I must stay as they were"""
    n, n_items = len(users), scorer.n_items
    out = torch.full((n + 1, n_items + slack), SENTINEL, dtype=torch.float32, device="cuda")
    got = scorer.score(dev(np.asarray(users, dtype=np.int64)), out=out)
    assert got is out
    x = out.cpu().numpy()
    assert (x[n] == SENTINEL).all() and (x[:, n_items:] == SENTINEL).all()      # the row past n and the columns past n_items are untouched
    return x[:n, :n_items]


@pytest.mark.parametrize("weighted", (False, True))
def test_equal_to_the_yardstick_bit_for_bit(weighted):
    index, host = indexes()
    csr, w = histories()
    w = w if weighted else None
    assert (host.nbr[:, 299:] == -1).all() and (host.nbr[:, :299] >= 0).all()
    users = np.array(list(range(20)) + [EMPTY, USER_NUM], dtype=np.int64)
    live = np.arange(20)
    for m in MS:
        want = item_knn_scores_host(host, csr, live, w, m)
        assert not np.isnan(want).any()
        scorer = ItemKnnScorer(index, csr, USER_NUM, w, m)
        for n in BATCHES:
            for slack in (0, 3):                             # a row stride of 303 floats: the rows begin at every alignment mod 16 bytes
                got = fused(scorer, users[:n], slack)
                k = min(n, 20)
                assert np.array_equal(bits(got[:k]), bits(want[:k])), (m, n, slack)
                assert np.isnan(got[k:]).all(), (m, n, slack)      # an empty user and an id outside the CSR: rows of NaN
    z = fused(ItemKnnScorer(index, csr, USER_NUM, w, 1), [0, 9])      # one history item, m = 1: one listed candidate, +0.0 everywhere else
    assert (np.count_nonzero(z, axis=1) == 1).all() and not np.signbit(z[z == 0]).any()
    assert np.isnan(fused(ItemKnnScorer(index, csr, USER_NUM, w), [EMPTY, -1, 2 ** 40])).all()      # a call with no live row at all


def test_the_tile_edges():
    """catalogues of exactly one tile, one item more, and two tiles and three items; users whose histories hold item 0, the last item of a
    tile and the first of the next, and items that LIST those candidates and the last one of the catalogue"""
    tile = int(_lib.hip().pmgt_knn_score_tile())
    assert tile >= 64 and tile % 4 == 0
    for n_items in (tile, tile + 1, 2 * tile + 3):
        table = np.random.default_rng(n_items).standard_normal((n_items, 8)).astype(np.float32)
        index = build_item_knn(dev(table), 16)
        host = index.host()
        edges = [c for c in (0, tile - 1, tile, 2 * tile - 1, 2 * tile, n_items - 1) if c < n_items]
        listers = []
        for c in edges:
            rows = np.nonzero((host.nbr == c).any(axis=1))[0]
            assert len(rows), c                              # (about 16 items list a candidate: the table lists every edge)
            listers.append(int(rows[0]))
        rng = np.random.default_rng(5)
        lists = [[c for c in (0, tile - 1, tile) if c < n_items], listers, listers[::2] + [0], rng.choice(n_items, 40, replace=False).tolist(),
                 [n_items - 1] + listers[1::2]]
        pairs = np.array([(u, i) for u, mine in enumerate(lists) for i in sorted(set(mine))], dtype=np.int64)
        weights = rng.uniform(0.5, 2.0, size=len(pairs)).astype(np.float32)
        for w in (None, weights):
            want = item_knn_scores_host(host, pairs, np.arange(5), w)
            assert all((want[1:, c] != 0).any() for c in edges)      # every edge candidate gets a term
            for slack in (0, 1):
                got = fused(ItemKnnScorer(index, pairs, 5, w), np.arange(5), slack)
                assert np.array_equal(bits(got), bits(want)), (n_items, w is None, slack)


def test_independent_of_the_batch_repeatable_and_the_prefix_property():
    index, host = indexes()
    csr, w = histories()
    for weights in (None, w):
        scorer = ItemKnnScorer(index, csr, USER_NUM, weights, 64)
        for u in (5, 4, 16, 0):                              # 300, 65, 20 items and one
            alone = fused(scorer, [u])
            for users in ([u] + list(range(20)), list(range(19)) + [u], [1, u, 2, u], [EMPTY, u, USER_NUM], [8, 17, u, 5, 8]):
                x = fused(scorer, users)
                for r in np.nonzero(np.array(users) == u)[0]:
                    assert np.array_equal(bits(x[r]), bits(alone[0])), (u, users)
        users = list(range(20)) + [3, 3]
        assert np.array_equal(bits(fused(scorer, users)), bits(fused(scorer, users)))      # two calls in a row
        # the scores of truncated(m2) are those of an index built at m2 (the device scores do not depend on the batch: any batch_items)
        for m2, batch in ((1, 300), (5, 41), (64, 7)):
            small = build_item_knn(dev(U.normal_table(D, 29)), m2, batch_items=batch)
            cut = index.truncated(m2)
            assert torch.equal(small.nbr, cut.nbr) and torch.equal(small.sim.view(torch.int32), cut.sim.view(torch.int32)) and cut.stride == 400
            a = fused(ItemKnnScorer(cut, csr, USER_NUM, weights), range(20))
            b = fused(ItemKnnScorer(small, csr, USER_NUM, weights), range(20))
            assert np.array_equal(bits(a), bits(b)), m2


def test_the_whole_neighbourhood_is_the_history_kernels_mean_times_the_length():
    """m = I - 1 keeps every other item: outside H(u) the sum is pmgt_history_score's mean times len (1, 2 and 4: exact), by value"""
    table = dev(U.normal_table(D, 29))
    index, _ = indexes()
    rng = np.random.default_rng(17)
    lengths = (1, 2, 4, 4, 2, 1)
    pairs = np.array([(u, int(i)) for u, n in enumerate(lengths) for i in rng.choice(N_ITEMS, size=n, replace=False)], dtype=np.int64)
    users = np.arange(len(lengths))
    knn = fused(ItemKnnScorer(index, pairs, len(lengths), m=N_ITEMS - 1), users)
    mean = fused(HistoryScorer(table, pairs, len(lengths), "mean", "cosine"), users)
    for u, n in enumerate(lengths):
        outside = np.ones(N_ITEMS, dtype=bool)
        outside[pairs[pairs[:, 0] == u, 1]] = False
        assert outside.sum() == N_ITEMS - n and np.array_equal(knn[u, outside], mean[u, outside] * np.float32(n)), u


def test_same_lists_ranks_and_metrics_on_both_impls():
    index, host = indexes()
    csr, w = histories()
    rng = np.random.default_rng(2)
    held = []
    for u in range(USER_NUM):
        mine = set(csr[1][csr[0][u]: csr[0][u + 1]].tolist())
        if 0 < len(mine) < N_ITEMS:
            held += [(u, int(j)) for j in rng.permutation([j for j in range(N_ITEMS) if j not in mine])[:2]]
    held = np.array(held, dtype=np.int64)
    most = np.array([(SHORT, j) for j in range(N_ITEMS) if j not in (7, 250)], dtype=np.int64)      # user 21 keeps two eligible items
    for weights in (None, w):
        for kw in (dict(m=5), dict(batch_users=7), dict(m=64, exclude=None, users=[19, 21, 3, 19]), dict(m=130, exclude=held, batch_users=5),
                   dict(m=5, exclude=most, users=[SHORT, 2])):
            a = recommend_item_knn(index, csr, k=20, weights=weights, impl="device", **kw)
            b = recommend_item_knn(index, csr, k=20, weights=weights, impl="host", **kw)      # (on the index copied from the device)
            assert a[0].dtype == np.int64 and np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])), kw
        short = recommend_item_knn(index, csr, k=20, m=5, weights=weights, exclude=most, users=[SHORT])
        assert sorted(short[0][0, :2].tolist()) == [7, 250] and (short[0][0, 2:] == -1).all() and np.isneginf(short[1][0, 2:]).all()
        full = recommend_item_knn(index, csr, users=[5], k=5, weights=weights)
        assert (full[0] == -1).all()                         # user 5 has everything: nothing is eligible
        for kw in (dict(m=64), dict(m=(1, 5, 64, 400), batch_users=7), dict(m=(5,), exclude=None)):
            ra, rb = (evaluate_item_knn(index, csr, held, ks=(1, 10, 20), weights=weights, impl=impl, per_user=True, **kw)
                      for impl in ("device", "host"))
            many = isinstance(kw["m"], tuple)
            assert not many or list(ra) == list(kw["m"])
            for (sa, pa), (sb, pb) in (zip(ra.values(), rb.values()) if many else ((ra, rb),)):
                assert sa == sb and set(pa) == set(pb)
                for key in ("users", "n_pos", "ranks", "indptr", "items", "rr"):
                    assert np.array_equal(pa[key], pb[key]), key
                for key in ("ndcg", "recall", "hit"):
                    for k in (1, 10, 20):
                        assert np.array_equal(pa[key][k], pb[key][k]), (key, k)
        sweep = evaluate_item_knn(index, csr, held, m=(5, 64), weights=weights)
        assert sweep == {m: evaluate_item_knn(index, csr, held, m=m, weights=weights) for m in (5, 64)}
    # a table in the first place: the index is built on the device with m (default 64)
    t = U.planted_table()
    hist = np.array([(c, 5 * c + a) for c in range(8) for a in (0, 2, 3)], dtype=np.int64)
    found, _ = recommend_item_knn(dev(t), hist, k=4, m=4)
    assert all(sorted(found[c, :2].tolist()) == [5 * c + 1, 5 * c + 4] for c in range(8))
    res = evaluate_item_knn(np.array(t), hist, [(c, 5 * c + a) for c in range(8) for a in (1, 4)])      # a numpy table is uploaded once
    assert res["r10"] == 1.0 and res["mrr"] == 1.0 and res["users"] == 8 and res["pairs"] == 16


def test_an_index_from_elsewhere_runs_on_the_device():
    """arrays that no builder made (a host index is uploaded once, device tensors are checked on the host): the rows written out by hand"""
    nbr = np.array([[1, 2], [0, 2], [1, 0], [2, -1], [0, 1]], dtype=np.int32)
    sim = np.array([[0.5, 0.25], [0.5, 0.125], [0.75, 0.25], [2.0, -np.inf], [1.0, -1.0]], dtype=np.float32)
    hist = [(0, 3), (0, 0), (1, 4), (1, 1), (1, 2)]
    want = np.array([[0.0, 0.5, 2.25, 0.0, 0.0], [1.75, -0.25, 0.125, 0.0, 0.0]], dtype=np.float32)
    for index in (ItemKnnIndex(nbr, sim, 5), ItemKnnIndex(dev(nbr), dev(sim), 5)):
        assert np.array_equal(bits(fused(ItemKnnScorer(index, hist, 2), [0, 1], slack=2)), bits(want))
    with pytest.raises(ValueError, match="1 of 5 rows repeat a neighbour id"):
        ItemKnnIndex(dev(np.where(np.arange(10).reshape(5, 2) == 1, 1, nbr).astype(np.int32)), dev(sim), 5)
    with pytest.raises(ValueError, match="knn_score: m = 3 is larger than the 2 neighbours"):
        ItemKnnScorer(ItemKnnIndex(nbr, sim, 5), hist, 2, m=3)
    s = ItemKnnScorer(ItemKnnIndex(nbr, sim, 5), hist, 2)
    with pytest.raises(ValueError, match="knn_score: users must be a contiguous int64 tensor"):
        s.score(dev(np.array([0, 1], dtype=np.int32)))
    with pytest.raises(ValueError, match=r"out must be a contiguous fp32 tensor \[>= 2, >= 5\]"):
        s.score(dev(np.array([0, 1], dtype=np.int64)), out=torch.empty(2, 4, device="cuda"))


def test_the_entry_ids_it_never_dereferences_and_its_refusals():
    index, host = indexes()
    csr, _ = histories()
    lib = _lib.hip()
    s = ItemKnnScorer(index, csr, USER_NUM, m=64)
    q = dev(np.array([1, 0], dtype=np.int64))
    out = torch.full((2, N_ITEMS), SENTINEL, device="cuda")
    args = lambda **kw: [kw.get("nbr", index.nbr.data_ptr()), kw.get("sim", index.sim.data_ptr()), kw.get("idx_stride", 400), kw.get("m", 64),
                         kw.get("ptr", s._indptr.data_ptr()), kw.get("items", s._items.data_ptr()), kw.get("weights", 0),
                         kw.get("users", q.data_ptr()), kw.get("n", 2), kw.get("user_num", USER_NUM), kw.get("n_items", N_ITEMS),
                         kw.get("out", out.data_ptr()), kw.get("stride", N_ITEMS), _lib.stream()]
    for kw, text in ((dict(m=0), "m = 0 outside"), (dict(m=1025, idx_stride=2048), "m = 1025 outside"), (dict(m=65, idx_stride=64), "idx_stride = 64 below m = 65"),
                     (dict(n=0), "n = 0 users outside"), (dict(n=(1 << 20) + 1), "users outside"), (dict(n_items=0), "0 items outside"),
                     (dict(n_items=2 ** 31 - 1, stride=2 ** 31), "items outside"), (dict(user_num=0), "user_num = 0 below 1"),
                     (dict(stride=299), "row_stride = 299 below"), (dict(nbr=0), "NULL buffer"), (dict(sim=0), "NULL buffer"),
                     (dict(ptr=0), "NULL buffer"), (dict(items=0), "NULL buffer"), (dict(users=0), "NULL buffer"), (dict(out=0), "NULL buffer"),
                     (dict(nbr=index.nbr.data_ptr() + 2), "misaligned buffer"), (dict(weights=index.sim.data_ptr() + 1), "misaligned buffer"),
                     (dict(users=q.data_ptr() + 4), "misaligned buffer"), (dict(ptr=s._indptr.data_ptr() + 4), "misaligned buffer"),
                     (dict(out=out.data_ptr() + 2), "misaligned buffer")):
        assert lib.pmgt_knn_score(*args(**kw)) == -2 and text in lib.pmgt_last_error().decode(), kw
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()             # nothing was launched, nothing written
    assert lib.pmgt_knn_score(*args()) == 0                  # (the same arguments unchanged are taken)
    whole = out.cpu().numpy()
    assert np.array_equal(bits(whole), bits(item_knn_scores_host(host, csr, [1, 0], m=64)))
    # a neighbour id >= n_items is skipped: the same index read as a catalogue of 200 items gives the first 200 columns of the whole rows
    low = history_of([[3, 150], [199]])
    cut = torch.full((2, 203), SENTINEL, device="cuda")
    ok = lib.pmgt_knn_score(*args(ptr=low[0].data_ptr(), items=low[1].data_ptr(), user_num=2, n_items=200, out=cut.data_ptr(), stride=203))
    want = item_knn_scores_host(host, [(0, 3), (0, 150), (1, 199)], [1, 0], m=64)
    got = cut.cpu().numpy()
    assert ok == 0 and np.array_equal(bits(got[:, :200]), bits(want[:, :200])) and (got[:, 200:] == SENTINEL).all()
    # a history item outside [0, n_items) is never dereferenced: it makes the whole row NaN, wherever it stands in the list
    for bad_list in ([N_ITEMS, 5], [5, -1], [5, 6, 7, 8, 2 ** 31 - 1], [-(2 ** 31)]):
        wild = history_of([bad_list, [3, 150]])
        rows = torch.full((2, N_ITEMS), SENTINEL, device="cuda")
        assert lib.pmgt_knn_score(*args(ptr=wild[0].data_ptr(), items=wild[1].data_ptr(), user_num=2, out=rows.data_ptr())) == 0
        rows = rows.cpu().numpy()                            # users [1, 0]: row 0 is the clean user, row 1 the one with the id outside
        assert np.isnan(rows[1]).all() and np.array_equal(bits(rows[0]), bits(want[1]))


def history_of(lists):
    """a raw CSR on the device, as the C entry reads it: unchecked"""
    indptr = np.zeros(len(lists) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=indptr[1:])
    return dev(indptr), dev(np.concatenate(lists).astype(np.int32))
