"""pmgt_topk_rows against topk_host, EXACTLY: items, scores (bit pattern) and flags, over row lengths on the wave / workgroup edges, tie-heavy
and all-equal rows, every kind of exclusion list, repeated users, k above the row length, slack past the row that must not be read."""
import ctypes as C

import numpy as np
import pytest
import torch

from pmgt_amd.recommend import TopkRows, topk_host

pytestmark = pytest.mark.gpu

TIE_VALUES = np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, 2.0, np.inf], dtype=np.float32)
KS = (1, 10, 100, 1024)
USERS = 6
# row length -> rows: every n of {1, 3, 130} meets short and long rows (the host yardstick of 130 x 70 001 alone would take the test's time)
CASES = [(1, 3), (63, 130), (64, 1), (65, 130), (257, 3), (5000, 130), (70001, 3), (70001, 1), (257, 130)]


def make_scores(n, n_items, seed):
    """Rows in turn: the tie-heavy value set, all equal, continuous; three floats of NaN slack behind every row."""
    rng = np.random.default_rng(seed)
    x = np.full((n, n_items + 3), np.nan, dtype=np.float32)
    for r in range(n):
        if r % 3 == 0:
            x[r, :n_items] = TIE_VALUES[rng.integers(0, len(TIE_VALUES), size=n_items)]
        elif r % 3 == 1:
            x[r, :n_items] = np.float32(0.25)
        else:
            x[r, :n_items] = rng.standard_normal(n_items).astype(np.float32)
    return x


def make_csr(x, users, n_items, k, seed):
    """User 0: the items that would win the first row that user has; 1: the whole row; 2 and 5: nothing; 3: exactly I - k items (none when
    k >= I); 4: a few items with duplicates."""
    rng = np.random.default_rng(seed)
    first = {int(u): r for r, u in reversed(list(enumerate(users)))}
    winners = topk_host(x[first.get(0, 0): first.get(0, 0) + 1, :n_items], min(5, n_items))[0][0]
    few = rng.integers(0, n_items, size=7)
    lists = [winners[winners >= 0], np.arange(n_items), np.zeros(0, np.int64), rng.permutation(n_items)[: max(n_items - k, 0)],
             np.concatenate([few, few[:3]]), np.zeros(0, np.int64)]
    indptr = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64)
    return indptr, np.concatenate(lists).astype(np.int32)


def same(got, want):
    return np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)) and \
        np.array_equal(got[2].view(np.uint32), want[2])


def fetch(out):
    return tuple(t.cpu().numpy() for t in out)


@pytest.mark.parametrize("n_items,n", CASES)
def test_equals_topk_host_exactly(n_items, n):
    x = make_scores(n, n_items, seed=n_items + n)
    users = ((np.arange(n) // 2) + n_items) % USERS          # users come twice in a batch
    xd = torch.from_numpy(x).cuda()
    ud = torch.from_numpy(users).cuda()
    for k in KS:
        indptr, items = make_csr(x, users, n_items, k, seed=k)
        picker = TopkRows("cuda", n, n_items, k, indptr, items, USERS)
        got = fetch(picker.select(xd, ud))
        want = topk_host(x[:, :n_items], k, indptr, items, users)
        assert same(got, want), (n_items, n, k)
        assert same(fetch(picker.select(xd, ud)), got), "a second identical call returns other bytes"
        free = fetch(TopkRows("cuda", n, n_items, k).select(xd))
        assert same(free, topk_host(x[:, :n_items], k)), (n_items, n, k, "no exclusion")
        assert not np.isnan(free[1][1::3]).any()              # the NaN slack past the row was not read (the tie rows hold no NaN either)
    if n > 1:                                                 # all-equal rows: 0, 1, 2, ... minus the exclusions
        u = int(users[1])
        gone = set(items[indptr[u]: indptr[u + 1]].tolist())
        left = [j for j in range(n_items) if j not in gone][:KS[-1]]
        assert got[0][1, :len(left)].tolist() == left and (got[0][1, len(left):] == -1).all()


def test_nan_among_the_eligible_sets_the_flag_and_ranks_first():
    x = np.linspace(-1, 1, 3 * 70, dtype=np.float32).reshape(3, 70)
    x[0, 17] = x[1, 17] = np.nan
    indptr = np.array([0, 0, 1, 1], dtype=np.int64)          # user 1 has item 17 excluded
    items = np.array([17], dtype=np.int32)
    users = np.array([0, 1, 2])
    got = fetch(TopkRows("cuda", 3, 70, 4, indptr, items, 3).select(torch.from_numpy(x).cuda(), torch.from_numpy(users).cuda()))
    assert same(got, topk_host(x, 4, indptr, items, users))
    assert got[2].view(np.uint32).tolist() == [1, 0, 0] and got[0][0, 0] == 17 and np.isnan(got[1][0, 0])


def test_refusals_return_minus_two_and_write_nothing():
    from pmgt_amd import _lib
    lib = _lib.hip()
    n, n_items, k = 4, 50, 8
    x = torch.randn(n, n_items, device="cuda")
    users = torch.zeros(n, dtype=torch.int64, device="cuda")
    indptr = torch.zeros(3, dtype=torch.int64, device="cuda")
    excl = torch.zeros(4, dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.pmgt_topk_workspace_bytes(n, n_items), dtype=torch.uint8, device="cuda")
    oi = torch.full((n, k), 7777, dtype=torch.int32, device="cuda")
    osc = torch.full((n, k), 7777.0, device="cuda")
    fl = torch.full((n,), 7777, dtype=torch.int32, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: t.data_ptr()
    ok = [p(x), n_items, n, n_items, k, p(users), p(indptr), p(excl), 2, 4, p(ws), p(oi), p(osc), p(fl), st]

    def call(**kw):
        names = ["scores", "row_stride", "n", "n_items", "k", "users", "indptr", "excluded", "user_num", "n_excluded", "workspace", "out_items",
                 "out_scores", "out_flags", "stream"]
        a = list(ok)
        for key, v in kw.items():
            a[names.index(key)] = v
        return lib.pmgt_topk_rows(*a)

    bad = [dict(k=0), dict(k=1025), dict(n_items=0), dict(n_items=2 ** 31 - 1), dict(n=0), dict(row_stride=n_items - 1), dict(scores=0),
           dict(workspace=0), dict(out_items=0), dict(out_scores=0), dict(out_flags=0), dict(scores=p(x) + 2), dict(workspace=p(ws) + 4),
           dict(users=0), dict(user_num=0), dict(excluded=0), dict(n_excluded=-1), dict(indptr=p(indptr) + 4)]
    assert [call(**b) for b in bad] == [-2] * len(bad)
    assert lib.pmgt_topk_workspace_bytes(0, 5) < 0 and lib.pmgt_topk_workspace_bytes(5, 0) < 0 and lib.pmgt_topk_workspace_bytes(5, 2 ** 31 - 1) < 0
    assert lib.pmgt_topk_workspace_bytes(2 ** 31 - 1, 2 ** 31 - 2) < 0            # the byte count would not fit
    torch.cuda.synchronize()
    assert (oi == 7777).all() and (osc == 7777.0).all() and (fl == 7777).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert not (oi == 7777).any() and not (fl == 7777).any()
    for bad_k in (0, 1025):
        with pytest.raises(ValueError, match="k ="):
            TopkRows("cuda", n, n_items, bad_k)
