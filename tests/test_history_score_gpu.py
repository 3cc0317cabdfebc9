"""pmgt_history_score against its unfused composition -- ItemSimScorer.score of the history items, copied out and reduced in numpy as the
score is defined --, compared with ==: s(i, j) already exists on the device with bits that do not depend on the batch, so no tolerance is
needed.  Then what the definition buys (independent of the batch, a NaN stays where it belongs, nothing past n_items is written),
recommend_from_history / evaluate_history on both impls, and the refusals."""
import functools

import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd import history as H
from pmgt_amd.history import HistoryScorer, evaluate_history, history_csr, recommend_from_history, reduce_history
from pmgt_amd.similar import METRICS, ItemSimScorer
from tests import item_sim_util as U

pytestmark = pytest.mark.gpu

SENTINEL = 7777.0
AGGS = ("mean", "max")
N_ITEMS = 300
DS = (1, 33, 64, 130)
# the history lengths of users 0 .. 39: a chunk of the kernel is 128 rows.  All 300 items at the first and the last slot of a group of 16,
# at the first slot of the next (the end of a batch of 17) and at the end of the batch of 40; 129 in the middle of a group.  The kernel's
# group is 48 slots: GROUPS below puts these users at the first, a middle and the last slot of such a group and at the end of a longer batch
LENGTHS = (300, 1, 2, 31, 32, 33, 127, 129, 128, 5, 1, 64, 3, 96, 2, 300,
           300, 7, 1, 33, 128, 2, 129, 31, 127, 32, 10, 300, 1, 1, 65, 4,
           20, 2, 128, 129, 3, 1, 127, 300)
EMPTY, SHORT = 40, 41                                        # user 40 and 42 have no history, 41 has four items, 43 one
USER_NUM = 44
BATCHES = (1, 17, 40)
GROUP = 48                                                   # the slots of a workgroup (HS_G of ops/history_score.hip)
# 100 slots = two groups and a part: a 300-item user at slot 0, 24, 47 (the last of a group), 48 (the first of the next), 95, 96 and 99
GROUPS = np.array([{0: 0, 24: 15, 47: 16, 48: 27, 95: 39, 96: 0, 99: 15}.get(r, 1 + r % 38) for r in range(100)])


@functools.lru_cache(maxsize=None)
def histories():
    """the history CSR over USER_NUM users, every list ascending without duplicates; read-only"""
    rng = np.random.default_rng(11)
    lists = [np.sort(rng.choice(N_ITEMS, size=n, replace=False)) for n in LENGTHS + (0, 4, 0, 1)]
    indptr = np.zeros(USER_NUM + 1, dtype=np.int64)
    np.cumsum([len(x) for x in lists], out=indptr[1:])
    items = np.concatenate(lists).astype(np.int32)
    indptr.setflags(write=False)
    items.setflags(write=False)
    return indptr, items


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def fused(table, users, agg, metric, slack=0, csr=None):
    """the kernel's rows [len(users), I]; with `slack`, into a wider buffer whose columns past I must stay as they were"""
    scorer = HistoryScorer(dev(table), csr or histories(), USER_NUM, agg, metric)
    n, n_items = len(users), len(table)
    out = torch.full((n + 1, n_items + slack), SENTINEL, dtype=torch.float32, device="cuda")
    got = scorer.score(dev(np.asarray(users, dtype=np.int64)), out=out)
    assert got is out
    x = out.cpu().numpy()
    assert (x[n] == SENTINEL).all() and (x[:, n_items:] == SENTINEL).all()      # the row past n and the canary past n_items are untouched
    return x[:n, :n_items]


def unfused(table, users, agg, metric):
    """THE YARDSTICK: ItemSimScorer.score of the users' history items in one call, copied out, then the reduction in numpy"""
    indptr, items = histories()
    flat = np.concatenate([items[indptr[u]: indptr[u + 1]] for u in users]).astype(np.int64)
    rows = ItemSimScorer(dev(table), metric).score(dev(flat)).cpu().numpy()
    out, at = np.empty((len(users), len(table)), dtype=np.float32), 0
    for r, u in enumerate(users):
        n = int(indptr[u + 1] - indptr[u])
        out[r] = reduce_history(rows[at: at + n], agg)
        at += n
    return out


@pytest.mark.parametrize("d", DS)
def test_equal_to_the_unfused_composition(d):
    table = U.normal_table(d, 29)
    users = np.arange(40)
    for metric in METRICS:
        for agg in AGGS:
            want = unfused(table, users, agg, metric)
            assert not np.isnan(want).any()
            for n in BATCHES:
                got = fused(table, users[:n], agg, metric, slack=3)
                assert np.array_equal(bits(got), bits(want[:n])), (metric, agg, n)
            for n in (GROUP, GROUP + 1, len(GROUPS)):        # a full group, one slot more, two groups and a part
                got = fused(table, GROUPS[:n], agg, metric, slack=1)
                assert np.array_equal(bits(got), bits(want[GROUPS[:n]])), (metric, agg, n)


def test_the_catalogue_cut_and_the_tile_edges():
    """fewer items than a tile, one more than a tile, and the scores of a shorter table are those of the longer one for the pairs it holds"""
    table = U.normal_table(33, 29)
    for cut in (1, 127, 129):
        rng = np.random.default_rng(cut)
        lists = [np.sort(rng.choice(cut, size=min(cut, n), replace=False)) for n in (1, 2, 5, 129, 3)]
        indptr = np.zeros(USER_NUM + 1, dtype=np.int64)
        indptr[1:6] = np.cumsum([len(x) for x in lists])
        indptr[6:] = indptr[5]
        csr = (indptr, np.concatenate(lists).astype(np.int32))
        for metric in METRICS:
            rows = ItemSimScorer(dev(table), metric).score(dev(np.arange(cut, dtype=np.int64))).cpu().numpy()[:, :cut]     # the longer table's
            for agg in AGGS:
                got = fused(table[:cut], np.arange(5), agg, metric, slack=2, csr=csr)
                want = np.stack([reduce_history(rows[x], agg) for x in lists])
                assert np.array_equal(bits(got), bits(want)), (cut, metric, agg)


def test_independent_of_the_batch_and_repeatable():
    table = U.normal_table(64, 29)
    for metric in METRICS:
        for agg in AGGS:
            for u in (5, 7, 15, 30):                         # 33, 129, 300 and 65 items
                alone = fused(table, [u], agg, metric)
                calls = ([u] + list(range(20)), list(range(16, 35)) + [u], [1, u, 2, u], [0, u, 39], [0, 15, 16, 27, u, 39, 0],
                         list(GROUPS[:47]) + [u, u] + list(GROUPS[:30]))      # the last slot of a group and the first of the next
                for users in calls:
                    x = fused(table, users, agg, metric)
                    for r in np.nonzero(np.array(users) == u)[0]:
                        assert np.array_equal(bits(x[r]), bits(alone[0])), (metric, agg, u, users)
            users = list(range(40)) + [3, 3]
            assert np.array_equal(bits(fused(table, users, agg, metric)), bits(fused(table, users, agg, metric)))      # two runs of one call


def test_a_nan_stays_in_its_column_and_in_the_rows_of_the_users_holding_it():
    indptr, items = histories()
    clean = U.normal_table(33, 29)
    x_item = int(items[indptr[SHORT]])                       # an item of user 41 (and of every 300-item user, and of some others)
    table = np.array(clean)
    table[x_item, 7] = np.nan
    users = np.array(list(range(40)) + [SHORT, 43], dtype=np.int64)
    holds = np.array([x_item in items[indptr[u]: indptr[u + 1]] for u in users])
    assert holds[0] and holds[40] and not holds.all()
    want = np.zeros((len(users), N_ITEMS), bool)
    want[holds] = True
    want[:, x_item] = True
    for metric in METRICS:
        for agg in AGGS:
            got = fused(table, users, agg, metric, slack=5)
            assert np.array_equal(np.isnan(got), want), (metric, agg)
            ref = fused(clean, users, agg, metric)
            assert np.array_equal(bits(got)[~want], bits(ref)[~want]), (metric, agg)      # every other score: the bits without the NaN


def test_an_empty_history_and_a_user_outside_the_csr_are_never_read_their_rows_are_nan():
    table = U.normal_table(8, 29)
    users = np.array([3, EMPTY, USER_NUM, -1, 2 ** 40, 42, SHORT], dtype=np.int64)
    for agg in AGGS:
        x = fused(table, users, agg, "cosine", slack=4)
        assert np.isnan(x[1:6]).all() and not np.isnan(x[[0, 6]]).any()
        assert np.array_equal(bits(x[[0, 6]]), bits(fused(table, [3, SHORT], agg, "cosine")))
        assert np.isnan(fused(table, [EMPTY], agg, "dot")).all()      # a call with no row at all launches and writes NaN
    # a zero result of the max is +0.0; the mean of exact zeros too
    zero = np.zeros((N_ITEMS, 8), dtype=np.float32)
    zero[:, 0] = -1.0
    zero[::2] = 0
    for agg in AGGS:
        z = fused(zero, [0, 3], agg, "dot")
        assert (z[:, ::2] == 0).all() and not np.signbit(z[:, ::2]).any()


@pytest.mark.parametrize("d", (8, 33))
def test_exact_case_same_lists_ranks_and_metrics_on_both_impls(d):
    """the integer table is full of ties and every sum is exact: lists, scores, ranks and metrics agree between the device and the host"""
    table = U.integer_table(d)
    hist = histories()
    rng = np.random.default_rng(2)
    held = []
    for u in range(USER_NUM):
        mine = set(hist[1][hist[0][u]: hist[0][u + 1]].tolist())
        if 0 < len(mine) < N_ITEMS:
            held += [(u, int(j)) for j in rng.permutation([j for j in range(N_ITEMS) if j not in mine])[:2]]
    held = np.array(held, dtype=np.int64)
    for agg in AGGS:
        for kw in (dict(), dict(batch_users=17), dict(exclude=None, users=[39, 41, 3, 39]), dict(exclude=held, batch_users=5)):
            a = recommend_from_history(table, hist, k=20, agg=agg, metric="dot", impl="device", **kw)
            b = recommend_from_history(table, hist, k=20, agg=agg, metric="dot", impl="host", **kw)
            assert a[0].dtype == np.int64 and np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])), (agg, kw)
        full = recommend_from_history(table, hist, users=[0, 1], k=5, agg=agg, metric="dot")
        assert (full[0][0] == -1).all() and (full[1][0] == -np.inf).all() and (full[0][1] >= 0).all()      # user 0 has everything: nothing is eligible
        for kw in (dict(), dict(batch_users=7), dict(exclude=None)):
            (ra, pa), (rb, pb) = (evaluate_history(table, hist, held, ks=(1, 10, 20), agg=agg, metric="dot", impl=impl, per_user=True, **kw)
                                  for impl in ("device", "host"))
            assert ra == rb and set(pa) == set(pb)
            for key in ("users", "n_pos", "ranks", "indptr", "items", "rr"):
                assert np.array_equal(pa[key], pb[key]), key
            for key in ("ndcg", "recall", "hit"):
                for k in (1, 10, 20):
                    assert np.array_equal(pa[key][k], pb[key][k]), (key, k)


def test_end_to_end_on_the_planted_table():
    t = U.planted_table()
    hist = np.array([(c, 5 * c + a) for c in range(8) for a in (0, 2, 3)], dtype=np.int64)
    held = np.array([(c, 5 * c + a) for c in range(8) for a in (1, 4)], dtype=np.int64)
    for table in (np.array(t), dev(t)):                      # a numpy array is uploaded once; a device tensor is read in place
        for agg in AGGS:
            found, scores = recommend_from_history(table, hist, k=4, agg=agg)
            host_found, host_scores = recommend_from_history(t, hist, k=4, agg=agg, impl="host")
            assert np.array_equal(found, host_found) and np.abs(scores - host_scores).max() <= 2.0 ** -22
            assert all(sorted(found[c, :2].tolist()) == [5 * c + 1, 5 * c + 4] for c in range(8))
            assert float((scores[:, 1] - scores[:, 2]).min()) >= 0.7
            for kw in (dict(), dict(batch_users=3)):
                res, rec = evaluate_history(table, hist, held, agg=agg, per_user=True, **kw)
                assert list(res) == ["n10", "n20", "r10", "r20", "hr10", "hr20", "mrr", "users", "pairs"]
                assert res["r10"] == 1.0 and res["n10"] == 1.0 and res["hr10"] == 1.0 and res["mrr"] == 1.0
                assert res["users"] == 8 and res["pairs"] == 16 and sorted(rec["ranks"].tolist()) == [1] * 8 + [2] * 8
                assert res == evaluate_history(t, hist, held, agg=agg, impl="host")


def test_refusals_come_before_any_launch(monkeypatch):
    class NoLaunch:
        def __init__(self, *a, **kw):
            raise AssertionError("a scorer was built")
    monkeypatch.setattr(H, "HistoryScorer", NoLaunch)
    monkeypatch.setattr(H, "device_table", NoLaunch)
    t = dev(U.planted_table())
    hist = np.array([(c, 5 * c + a) for c in range(8) for a in (0, 2, 3) if c != 3], dtype=np.int64)
    hist = np.concatenate([hist, [(8, 1)]])
    held = np.array([(c, 5 * c + 1) for c in range(8) if c != 3], dtype=np.int64)
    for call in (lambda **kw: recommend_from_history(t, hist, **kw), lambda **kw: evaluate_history(t, hist, held, **kw)):
        with pytest.raises(ValueError, match="impl='gpu'"):
            call(impl="gpu")
        with pytest.raises(ValueError, match="metric='l2'"):
            call(metric="l2")
        with pytest.raises(ValueError, match="agg='sum'"):
            call(agg="sum")
        with pytest.raises(ValueError, match="batch_users = -1"):
            call(batch_users=-1)
        with pytest.raises(ValueError, match=r"exclude: excluded items in \[40, 40\] outside"):
            call(exclude=[(0, 40)])
    with pytest.raises(ValueError, match="k = 1025"):
        recommend_from_history(t, hist, k=1025)
    with pytest.raises(ValueError, match="recommend_from_history: 1 of 2 users have an empty history"):
        recommend_from_history(t, hist, users=[3, 4])
    with pytest.raises(ValueError, match=r"recommend_from_history: users in \[0, 9\] outside \[0, 9\)"):
        recommend_from_history(t, hist, users=[0, 9])
    with pytest.raises(ValueError, match=r"histories: history items in \[0, 40\] outside \[0, 40\)"):
        recommend_from_history(t, [(0, 0), (0, 40)])
    wide = torch.zeros(2, 1025, device="cuda")
    with pytest.raises(ValueError, match=r"recommend_from_history: d = 1025 outside \[1, 1024\]"):
        recommend_from_history(wide, [(0, 1)])
    with pytest.raises(ValueError, match=r"evaluate_history: d = 1025 outside \[1, 1024\]"):
        evaluate_history(wide, [(0, 1)], [(0, 0)])
    with pytest.raises(ValueError, match="the held-out set is empty"):
        evaluate_history(t, hist, [])
    with pytest.raises(ValueError, match="evaluate_history: 1 of 8 users have an empty history"):
        evaluate_history(t, hist, np.concatenate([held, [(3, 16)]]))
    with pytest.raises(ValueError, match="1 of 7 held-out pairs are also excluded"):
        evaluate_history(t, hist, held, exclude=[(0, 1)])
    with pytest.raises(ValueError, match="ks="):
        evaluate_history(t, hist, held, ks=())


def test_a_nan_among_the_eligible_scores_is_refused_by_the_flag_path():
    t = np.array(U.planted_table())
    t[4, 1] = np.nan
    hist = np.array([(c, 5 * c + a) for c in range(8) for a in (0, 2, 3)], dtype=np.int64)
    with pytest.raises(ValueError, match="recommend_from_history: 2 of 3 users have a NaN score among their eligible items"):
        recommend_from_history(dev(t), hist, users=[0, 1, 2], exclude=[(1, 4)])
    recommend_from_history(dev(t), hist, users=[1, 2], exclude=[(1, 4), (2, 4)])      # excluded for all: no error
    with pytest.raises(ValueError, match="evaluate_history: 7 of 7 users have a NaN score among their eligible items"):
        evaluate_history(dev(t), hist, [(c, 5 * c + 1) for c in range(1, 8)])


def test_refusals_of_the_scorer_and_the_entry():
    t = dev(U.planted_table())
    hist = [(0, 1), (0, 2), (1, 3)]
    with pytest.raises(ValueError, match="history_score: the table must be a contiguous fp32 tensor on a GPU"):
        HistoryScorer(t.cpu(), hist, 2)
    with pytest.raises(ValueError, match="history_score: the table must be a contiguous fp32 tensor on a GPU"):
        HistoryScorer(t.t(), hist, 2)
    with pytest.raises(ValueError, match="eps = 0.0 is not a positive finite number"):
        HistoryScorer(t, hist, 2, eps=0.0)
    with pytest.raises(ValueError, match="metric='l1'"):
        HistoryScorer(t, hist, 2, metric="l1")
    with pytest.raises(ValueError, match="agg='sum'"):
        HistoryScorer(t, hist, 2, agg="sum")
    with pytest.raises(ValueError, match="user_num = 0 must be a positive integer"):
        HistoryScorer(t, hist, 0)
    with pytest.raises(ValueError, match=r"histories: users in \[0, 1\] outside \[0, 1\)"):
        HistoryScorer(t, hist, 1)
    s = HistoryScorer(t, hist, 2)
    assert s.ids_name == "users" and s.n_items == 40 and s.user_num == 2
    q = dev(np.array([1, 0], dtype=np.int64))
    with pytest.raises(ValueError, match="history_score: users must be a contiguous int64 tensor"):
        s.score(q.int())
    with pytest.raises(ValueError, match=r"out must be a contiguous fp32 tensor \[>= 2, >= 40\]"):
        s.score(q, out=torch.empty(2, 39, device="cuda"))
    # the entry itself refuses what the surface would not pass on, before anything is launched
    lib = _lib.hip()
    out = torch.full((2, 40), SENTINEL, device="cuda")
    args = lambda **kw: [kw.get("table", t.data_ptr()), s.inv_norm.data_ptr(), kw.get("ptr", s._indptr.data_ptr()),
                         kw.get("items", s._items.data_ptr()), kw.get("users", q.data_ptr()), kw.get("n", 2), kw.get("user_num", 2),
                         kw.get("n_items", 40), kw.get("d", 8), kw.get("agg", 0), kw.get("out", out.data_ptr()), kw.get("stride", 40), _lib.stream()]
    for kw, text in ((dict(d=0), "d = 0 outside"), (dict(d=1025), "d = 1025 outside"), (dict(n=0), "n = 0 users outside"),
                     (dict(n=(1 << 20) + 1), "users outside"), (dict(n_items=0), "0 items outside"), (dict(user_num=0), "user_num = 0 below 1"),
                     (dict(stride=39), "row_stride = 39 below"), (dict(agg=2), "unknown agg 2"), (dict(agg=-1), "unknown agg -1"),
                     (dict(table=0), "NULL buffer"), (dict(ptr=0), "NULL buffer"), (dict(items=0), "NULL buffer"), (dict(users=0), "NULL buffer"),
                     (dict(out=0), "NULL buffer"), (dict(table=t.data_ptr() + 2), "misaligned buffer"),
                     (dict(users=q.data_ptr() + 4), "misaligned buffer"), (dict(ptr=s._indptr.data_ptr() + 4), "misaligned buffer")):
        assert lib.pmgt_history_score(*args(**kw)) == -2 and text in lib.pmgt_last_error().decode(), kw
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == SENTINEL).all()
    assert lib.pmgt_history_score(*args()) == 0              # (the same arguments unchanged are taken)
    torch.cuda.synchronize()
    assert not (out.cpu().numpy() == SENTINEL).any()
