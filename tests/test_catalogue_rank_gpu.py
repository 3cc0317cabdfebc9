"""pmgt_rank_heldout and pmgt_rank_heldout_reduce against heldout_ranks_host / catalogue_metrics_host, EXACTLY: ranks, flags, per-user
records and sums, over row lengths on the wave / workgroup edges, tie-heavy and all-equal rows, NaNs, every kind of exclusion list, users
with no and one held-out item, more held-out items than one chunk, slack past the row that must not be read, and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.catalogue_eval import catalogue_metrics_host, heldout_ranks_host
from pmgt_amd.metrics import discount_tables

pytestmark = pytest.mark.gpu

TIE_VALUES = np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, 2.0, np.inf], dtype=np.float32)
NAN, GONE = _lib.TOPK_FLAG_NAN, _lib.RANK_HELDOUT_FLAG_EXCLUDED
SENTINEL = 7777
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "catalogue_eval_48x300.npz")


def csr(lists):
    return (np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64),
            np.concatenate([np.asarray(l, dtype=np.int32) for l in lists] + [np.zeros(0, np.int32)]).astype(np.int32))


def make_scores(n, n_items, seed, slack=3):
    """Rows in turn: the tie-heavy value set, all equal, continuous, continuous with NaNs; `slack` floats of NaN behind every row."""
    rng = np.random.default_rng(seed)
    x = np.full((n, n_items + slack), np.nan, dtype=np.float32)
    for r in range(n):
        if r % 4 == 0:
            x[r, :n_items] = TIE_VALUES[rng.integers(0, len(TIE_VALUES), size=n_items)]
        elif r % 4 == 1:
            x[r, :n_items] = np.float32(0.25)
        else:
            x[r, :n_items] = rng.standard_normal(n_items).astype(np.float32)
            if r % 4 == 3:
                x[r, rng.integers(0, n_items, size=2)] = np.nan
    return x


def make_lists(n, n_items, seed):
    """Per user, by id mod 4 -- held-out: a few items, one item, many, none; by id mod 5 -- excluded: nothing, a few with duplicates in
    no order, many in order with duplicates, everything but the first held-out item, the first held-out item itself among others."""
    rng = np.random.default_rng(seed)
    held, excl = [], []
    for u in range(n):
        count = (int(rng.integers(2, 8)), 1, int(rng.integers(20, 40)), 0)[u % 4]
        h = rng.choice(n_items, size=min(count, n_items), replace=False)
        few = rng.integers(0, n_items, size=7)
        many = np.sort(rng.integers(0, n_items, size=min(2 * n_items, 90)))
        e = (np.zeros(0, np.int64), np.concatenate([few, few[:3]]), many,
             np.setdiff1d(np.arange(n_items), h[:1]) if len(h) else np.arange(n_items), np.concatenate([few, h[:1]]))[u % 5]
        held.append(np.sort(h))
        excl.append(e)
    return csr(held), csr(excl)


class Device:
    """The raw entries on device copies of a case; outputs start at a sentinel so that what a call leaves alone shows."""

    def __init__(self, x, n_items, users, held, excl, user_num):
        self.lib = _lib.hip()
        self.n, self.stride, self.n_items, self.user_num = x.shape[0], x.shape[1], n_items, user_num
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        self.x, self.users = dev(x), dev(np.asarray(users, dtype=np.int64))
        self.h_indptr, self.h_items = dev(held[0]), dev(held[1])
        self.e_indptr, self.e_items = (dev(excl[0]), dev(excl[1])) if excl is not None else (None, None)
        self.ranks = torch.full((max(len(held[1]), 1),), -SENTINEL, dtype=torch.int32, device="cuda")
        self.flags = torch.full((self.n,), SENTINEL, dtype=torch.int32, device="cuda")
        self.n_held = len(held[1])
        self.st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def rank_args(self):
        p = lambda t: t.data_ptr() if t is not None and t.numel() else 0
        return [p(self.x), self.stride, self.n, self.n_items, p(self.users), p(self.e_indptr), p(self.e_items), self.user_num,
                len(self.e_items) if self.e_items is not None else 0, p(self.h_indptr), p(self.h_items), self.n_held, p(self.ranks),
                p(self.flags), self.st]

    def rank(self):
        assert self.lib.pmgt_rank_heldout(*self.rank_args()) == 0, self.lib.pmgt_last_error()
        return self.ranks.cpu().numpy()[: self.n_held], self.flags.cpu().numpy().view(np.uint32)

    def reduce_buffers(self, ks, who, who_flags):
        nk = len(ks)
        disc, idcg = discount_tables(ks[-1])
        self.ks_c = (C.c_int * nk)(*ks)
        self.disc, self.idcg = torch.from_numpy(disc).cuda(), torch.from_numpy(idcg).cuda()
        self.who = torch.from_numpy(np.asarray(who, dtype=np.int64)).cuda()
        self.who_flags = torch.from_numpy(np.ascontiguousarray(who_flags).view(np.int32)).cuda()
        self.records = torch.full((3 * nk + 1, len(who)), float(SENTINEL), dtype=torch.float64, device="cuda")
        self.header = torch.full((16,), float(SENTINEL), dtype=torch.float64, device="cuda")

    def reduce_args(self):
        p = lambda t: t.data_ptr()
        return [p(self.ranks), p(self.h_indptr), p(self.who), p(self.who_flags), len(self.who), self.user_num, self.n_held, self.ks_c,
                len(self.ks_c), p(self.disc), p(self.idcg), p(self.records), p(self.header), self.st]

    def reduce(self):
        assert self.lib.pmgt_rank_heldout_reduce(*self.reduce_args()) == 0, self.lib.pmgt_last_error()
        return self.records.cpu().numpy(), self.header.cpu().numpy()


def check_case(x, n_items, users, held, excl, user_num, ks=(1, 10, 20)):
    """One case end to end, bit for bit; returns the device's (ranks, flags) and the Device."""
    users = np.asarray(users, dtype=np.int64)
    want_r, want_f = heldout_ranks_host(x[:, :n_items], users, held, excl)
    d = Device(x, n_items, users, held, excl, user_num)
    got_r, got_f = d.rank()
    has = np.diff(held[0])[users] > 0
    reached = np.zeros(len(held[1]), dtype=bool)
    for u in users[has]:
        reached[held[0][u]: held[0][u + 1]] = True
    assert np.array_equal(got_r, np.where(reached, want_r, -SENTINEL)), "ranks"
    assert np.array_equal(got_f, np.where(has, want_f, SENTINEL).astype(np.uint32)), "flags"
    r2, f2 = d.rank()
    assert r2.tobytes() == got_r.tobytes() and f2.tobytes() == got_f.tobytes(), "a second identical call returns other bytes"
    if reached.all() and has.any():                          # every user with held-out items has a row: the metrics of the whole CSR
        m = catalogue_metrics_host(want_r, held[0], ks)
        row_of = {int(u): r for r, u in enumerate(users)}
        who_flags = np.array([want_f[row_of[int(u)]] for u in m["users"]], dtype=np.uint32)
        d.reduce_buffers(ks, m["users"], who_flags)
        rec, hdr = d.reduce()
        nk = len(ks)
        for i, k in enumerate(ks):
            assert rec[i].tobytes() == m["ndcg"][k].tobytes(), ("ndcg", k)
            assert rec[nk + i].tobytes() == m["recall"][k].tobytes(), ("recall", k)
            assert rec[2 * nk + i].tobytes() == m["hit"][k].tobytes(), ("hit", k)
            want = np.array([m["sums"]["ndcg"][k], m["sums"]["recall"][k], m["sums"]["hit"][k]])
            assert hdr[[i, 4 + i, 8 + i]].tobytes() == want.tobytes(), ("sums", k)
        assert rec[3 * nk].tobytes() == m["rr"].tobytes() and hdr[12] == m["sums"]["rr"]
        assert hdr.view(np.uint64)[13:].tolist() == [len(m["users"]), int(np.count_nonzero(who_flags & NAN)), int(np.count_nonzero(who_flags & GONE))]
        for g in range(3):
            assert (hdr[4 * g + nk: 4 * g + 4] == 0.0).all()
        rec2, hdr2 = d.reduce()
        assert rec2.tobytes() == rec.tobytes() and hdr2.tobytes() == hdr.tobytes(), "a second identical reduce returns other bytes"
    return got_r, got_f, d


@pytest.mark.parametrize("n_items", [1, 63, 65, 300, 1000])
@pytest.mark.parametrize("n", [1, 5, 67])
def test_equals_the_numpy_yardstick_exactly(n_items, n):
    x = make_scores(n, n_items, seed=n_items + n)
    held, excl = make_lists(n, n_items, seed=3 * n_items + n)
    users = np.random.default_rng(n).permutation(n)           # every user once: a row per user, in no order
    got_r, got_f, _ = check_case(x, n_items, users, held, excl, n)
    if n >= 5:
        assert got_f[users.tolist().index(4)] & GONE            # user 4: the first held-out item is excluded
    free, _, _ = check_case(x, n_items, users, held, None, n)             # no exclusion CSR: everything is eligible
    assert (free[free != -SENTINEL] >= 1).all()


def test_other_cut_offs_on_the_wave_edges():
    n, n_items = 9, 1500
    x = make_scores(n, n_items, seed=1, slack=0)
    rng = np.random.default_rng(2)
    held = csr([np.sort(rng.choice(n_items, size=600, replace=False)) for _ in range(n)])      # ranks on both sides of every cut-off
    check_case(x, n_items, np.arange(n), held, None, n, ks=(64, 65, 128, 1024))
    check_case(x, n_items, np.arange(n), held, None, n, ks=(1000,))


def test_more_held_out_items_than_one_chunk_and_long_exclusion_lists():
    n_items = 3000
    rng = np.random.default_rng(5)
    x = make_scores(3, n_items, seed=9)
    x[0, :n_items] = rng.standard_normal(n_items).astype(np.float32)
    x[0, 11] = np.nan
    big = rng.choice(n_items, size=_lib.RANK_HELDOUT_CHUNK + 1, replace=False)
    held = csr([np.sort(big), [5], rng.choice(n_items, size=2100, replace=False)])       # one item over a chunk; one; two chunks and a bit
    # longer than the row's thread count: in no order with duplicates (checked entry by entry), and in order with duplicates
    unordered = rng.integers(0, n_items, size=300)
    unordered[7] = big[0]
    excl = csr([unordered, np.sort(rng.integers(0, n_items, size=600)), np.zeros(0, np.int64)])
    got_r, got_f, _ = check_case(x, n_items, [0, 1, 2], held, excl, 3)
    assert got_f[0] & GONE and (got_r == 0).sum() >= 1
    check_case(x[[2, 0]], n_items, [2, 0], held, excl, 3)      # a user without a row: its places are left alone


def test_ties_nans_and_the_single_eligible_item():
    n_items = 40
    x = np.linspace(-1, 1, 4 * n_items, dtype=np.float32).reshape(4, n_items).copy()
    x[0, 17] = x[1, 17] = np.nan
    x = np.concatenate([x, np.full((4, 2), np.nan, dtype=np.float32)], axis=1)
    # user 0: the NaN is eligible; user 1: it is excluded; user 2: a held-out item is excluded; user 3: everything but item 5 is excluded
    excl = csr([[], [17], [3, 8], [j for j in range(n_items) if j != 5]])
    held = csr([[2, 17], [2], [3, 4], [5]])
    got_r, got_f, _ = check_case(x, n_items, np.arange(4), held, excl, 4, ks=(1, 10))
    assert got_f.tolist() == [NAN, 0, GONE, 0] and got_r.tolist() == [38, 1, 37, 0, 35, 1]
    # a duplicate in a held-out list gets the item's rank at both places
    dup = csr([[2, 2, 17], [], [], []])
    d = Device(x, n_items, np.arange(4), dup, excl, 4)
    r, f = d.rank()
    assert r.tolist() == [38, 38, 1] and f.tolist() == [NAN, SENTINEL, SENTINEL, SENTINEL]


def test_golden_fixture_against_the_reference():
    g = np.load(GOLDEN)
    U = 48
    got_r, got_f, d = check_case(g["scores"], 300, np.arange(U), (g["held_indptr"], g["held_items"]), (g["excl_indptr"], g["excl_items"]), U,
                                 ks=(10, 20))
    assert not got_f.any()
    rec, hdr = d.reduce()
    for i, k in enumerate((10, 20)):
        assert rec[i].tobytes() == g[f"n{k}_user"].tobytes() and rec[2 + i].tobytes() == g[f"r{k}_user"].tobytes(), k
        for got, want in ((hdr[i] / U, float(g[f"n{k}"])), (hdr[4 + i] / U, float(g[f"r{k}"]))):
            assert abs(got - want) <= U * 2.0 ** -52 * abs(want), (k, got, want)
    # the places are those of the reference's list
    for u in range(U):
        for h in range(g["held_indptr"][u], g["held_indptr"][u + 1]):
            if got_r[h] <= 100:
                assert g["predictions"][u, got_r[h] - 1] == g["held_items"][h]
            else:
                assert g["held_items"][h] not in g["predictions"][u]


def test_refusals_return_minus_two_and_write_nothing():
    n, n_items = 4, 50
    x = make_scores(n, n_items, seed=1, slack=0)
    held, excl = csr([[1, 2], [3], [4], [5, 6]]), csr([[7], [], [8, 9], []])
    d = Device(x, n_items, np.arange(n), held, excl, n)
    names = ["scores", "row_stride", "n", "n_items", "users", "indptr", "excluded", "user_num", "n_excluded", "held_indptr", "held_items",
             "n_heldout", "ranks", "flags", "stream"]

    def call(fn, ok, names, **kw):
        a = list(ok)
        for key, v in kw.items():
            a[names.index(key)] = v
        return fn(*a)

    ok = d.rank_args()
    p = lambda t: t.data_ptr()
    bad = [dict(n_items=0), dict(n_items=2 ** 31 - 1), dict(n=0), dict(row_stride=n_items - 1), dict(scores=0), dict(users=0), dict(held_indptr=0),
           dict(ranks=0), dict(flags=0), dict(held_items=0), dict(excluded=0), dict(n_excluded=-1), dict(n_heldout=-1), dict(user_num=0),
           dict(scores=p(d.x) + 2), dict(ranks=p(d.ranks) + 2), dict(flags=p(d.flags) + 1), dict(users=p(d.users) + 4),
           dict(indptr=p(d.e_indptr) + 4), dict(held_indptr=p(d.h_indptr) + 4), dict(held_items=p(d.h_items) + 2), dict(excluded=p(d.e_items) + 2)]
    assert [call(d.lib.pmgt_rank_heldout, ok, names, **b) for b in bad] == [-2] * len(bad)
    torch.cuda.synchronize()
    assert (d.ranks == -SENTINEL).all() and (d.flags == SENTINEL).all()
    got_r, got_f = d.rank()
    assert (got_r >= 1).all() and not (got_f == SENTINEL).any()
    # the reduce
    d.reduce_buffers((10, 20), np.arange(n), np.zeros(n, dtype=np.uint32))
    rnames = ["ranks", "held_indptr", "users", "flags", "n_users", "user_num", "n_heldout", "ks", "n_k", "disc", "idcg", "records", "header",
              "stream"]
    rok = d.reduce_args()
    down, zero, many, high = (C.c_int * 2)(20, 10), (C.c_int * 2)(0, 10), (C.c_int * 5)(1, 2, 3, 4, 5), (C.c_int * 2)(10, 1025)
    rbad = [dict(ranks=0), dict(held_indptr=0), dict(users=0), dict(disc=0), dict(idcg=0), dict(records=0), dict(header=0), dict(ks=None),
            dict(n_users=0), dict(user_num=0), dict(n_heldout=0), dict(n_k=0), dict(n_k=5, ks=many), dict(ks=down), dict(ks=zero), dict(ks=high),
            dict(ranks=p(d.ranks) + 2), dict(flags=p(d.who_flags) + 2), dict(users=p(d.who) + 4), dict(disc=p(d.disc) + 4),
            dict(records=p(d.records) + 4), dict(header=p(d.header) + 4)]
    assert [call(d.lib.pmgt_rank_heldout_reduce, rok, rnames, **b) for b in rbad] == [-2] * len(rbad)
    torch.cuda.synchronize()
    assert (d.records == SENTINEL).all() and (d.header == SENTINEL).all()
    assert call(d.lib.pmgt_rank_heldout_reduce, rok, rnames, flags=0) == 0      # no flags: nothing is counted
    torch.cuda.synchronize()
    assert not (d.records == SENTINEL).any() and d.header.cpu().numpy().view(np.uint64)[13:].tolist() == [n, 0, 0]


def test_the_device_classes():
    from pmgt_amd.catalogue_eval import CatalogueMetrics, HeldoutRanks
    g = np.load(GOLDEN)
    U = 48
    held, excl = (g["held_indptr"], g["held_items"]), (g["excl_indptr"], g["excl_items"])
    ranker = HeldoutRanks("cuda", 300, *held, U, *excl)
    xd, ud = torch.from_numpy(g["scores"]).cuda(), torch.arange(U, device="cuda")
    flags = torch.zeros(U, dtype=torch.int32, device="cuda")
    for lo in range(0, U, 7):                                 # in batches: the slices of users and flags
        ranker.rank(xd[lo: lo + 7], ud[lo: lo + 7], flags[lo: lo + 7])
    want_r, want_f = heldout_ranks_host(g["scores"], np.arange(U), held, excl)
    assert np.array_equal(ranker.ranks.cpu().numpy(), want_r) and not flags.any()
    cm = CatalogueMetrics("cuda", U + 5, (10, 20))           # room for more users than are reduced
    cm.reduce(ranker, ud, flags)
    st, pu = cm.statistic(), cm.per_user()
    m = catalogue_metrics_host(want_r, held[0], (10, 20))
    assert st["n_users"] == U and st["n_nan"] == 0 and st["n_excluded"] == 0
    for k in (10, 20):
        assert st["ndcg"][k] == m["sums"]["ndcg"][k] and st["recall"][k] == m["sums"]["recall"][k] and st["hit"][k] == m["sums"]["hit"][k]
        assert np.array_equal(pu["ndcg"][k], g[f"n{k}_user"]) and np.array_equal(pu["recall"][k], g[f"r{k}_user"])
    assert st["rr"] == m["sums"]["rr"] and np.array_equal(pu["rr"], m["rr"])
    with pytest.raises(ValueError, match="scores must be a contiguous fp32 device tensor"):
        ranker.rank(xd[:, :299], ud)
    with pytest.raises(ValueError, match="users must be a contiguous int64 device tensor"):
        ranker.rank(xd, ud[:5])
    with pytest.raises(ValueError, match="scores must be a contiguous fp32 device tensor"):
        ranker.rank(xd[0], ud[:1])                            # one-dimensional
    with pytest.raises(ValueError, match="nothing was reduced"):
        CatalogueMetrics("cuda", U, (10, 20)).per_user()
    with pytest.raises(ValueError, match="heldout: held-out items in"):
        HeldoutRanks("cuda", 10, *held, U)
    with pytest.raises(ValueError, match="ks="):
        CatalogueMetrics("cuda", U, (20, 10))
