"""recommend() end to end on the Deep & Cross Network: the device path (DcnScorer + TopkRows) against the host path (model.forward on pair
rows + topk_host) for scripts/run_dcn.sh's shape and for the widest MFMA shape, 80 users x 300 items.  The two sum a logit in different
orders, so the comparison is tests/test_recommend_ncf_model_gpu.py's: with s_h the host's full score rows and
tol = 4 max(max|s_h - o64|, 2^-22 max|o64|), o64 = dcn_scores_host in fp64, per user
  (a) the returned items are unique, in range, never excluded, and -1 exactly where the host pads;
  (b) the returned scores are non-increasing, equal-score neighbours in index order;
  (c) |score_dev - s_h[item]| <= tol;
  (d) every returned item has s_h[item] >= (k-th best eligible s_h) - 2 tol: the right set up to near-ties."""
import numpy as np
import pytest
import torch

from pmgt_amd.dcn_head import dcn_scores_host
from tests.dcn_score_util import EPS, ITEMS, USER_NUM, head_id
from tests.dcn_score_util import world as scored
from tests.dcn_util import torch_model

pytestmark = pytest.mark.gpu

N_ITEMS = ITEMS[-1]


@pytest.fixture(scope="module", params=[(16, 1, 4, True), (64, 2, 6, True)], ids=head_id)
def world(request):
    from pmgt_amd.recommend import dcn_host_scores, exclusion_csr
    head = request.param
    w = scored(head)["w"]
    model = torch_model({k: np.array(v) for k, v in w.items()}, head, device="cuda")
    rng = np.random.default_rng(11)
    # user 0 has nothing excluded, user 1 every item but three, the others 1 .. 24 items
    pairs = [(1, int(i)) for i in rng.permutation(N_ITEMS)[3:]]
    pairs += [(u, int(i)) for u in range(2, USER_NUM) for i in rng.choice(N_ITEMS, size=int(rng.integers(1, 25)), replace=False)]
    users = np.concatenate([np.arange(USER_NUM), [1, 0, USER_NUM - 1]])      # users come twice
    # a view of another buffer holding the model's item rows
    table = torch.cat([torch.zeros(1, head[0] << head[1], device="cuda"), model.item_embeddings.weight.detach()])[1:]
    model.eval()
    s_h = dcn_host_scores(model, table, users)
    o64 = dcn_scores_host(w, users, None, np.float64, EPS)
    tol = 4 * max(np.abs(s_h - o64).max(), 2.0 ** -22 * np.abs(o64).max())
    indptr, excl = exclusion_csr(pairs, USER_NUM, N_ITEMS)
    return dict(head=head, model=model, pairs=pairs, users=users, table=table, s_h=s_h, tol=tol, indptr=indptr, excl=excl)


@pytest.mark.parametrize("k", [1, 20, "above the item count"])
def test_device_path_against_host_path(world, k):
    from pmgt_amd.recommend import recommend
    model, users, s_h, tol, table = (world[x] for x in ("model", "users", "s_h", "tol", "table"))
    n_items = N_ITEMS
    k = n_items + 5 if isinstance(k, str) else k
    model.train()
    it_d, sc_d = recommend(model, None, users, k=k, exclude=world["pairs"], impl="device", table=table)
    it_h, sc_h = recommend(model, None, users, k=k, exclude=world["pairs"], impl="host", table=table)
    assert model.training                                     # the mode the caller had is restored
    assert it_d.dtype == np.int64 and sc_d.dtype == np.float32 and it_d.shape == sc_d.shape == (len(users), k)
    exact = 0
    for r, u in enumerate(users):
        gone = set(world["excl"][world["indptr"][u]: world["indptr"][u + 1]].tolist())
        live = it_d[r] >= 0
        got = it_d[r][live]
        # (a)
        assert np.array_equal(live, it_h[r] >= 0) and np.isneginf(sc_d[r][~live]).all() and (it_d[r][~live] == -1).all()
        assert len(set(got.tolist())) == len(got) and (got < n_items).all() and not (set(got.tolist()) & gone)
        assert live.sum() == min(k, n_items - len(gone))
        # (b)
        s = sc_d[r][live]
        assert (np.diff(s) <= 0).all() and (np.diff(got)[np.diff(s) == 0] > 0).all()
        # (c)
        assert np.abs(s.astype(np.float64) - s_h[r, got]).max(initial=0.0) <= tol
        # (d)
        elig = np.array([j for j in range(n_items) if j not in gone])
        if len(got):
            kth = np.sort(s_h[r, elig])[::-1][len(got) - 1]
            assert (s_h[r, got] >= kth - 2 * tol).all()
        exact += np.array_equal(it_d[r], it_h[r])
    print(f"{head_id(world['head'])} k = {k}: {exact} of {len(users)} users get exactly the host's item list (tol {tol:.3e})")
    assert (it_d[0] >= 0).sum() == min(k, n_items) and (it_d[1] >= 0).sum() == min(k, 3)      # nothing excluded / all but three


def test_batching_default_table_and_mode(world):
    from pmgt_amd.recommend import recommend
    model, users, pairs = world["model"], world["users"], world["pairs"]
    model.eval()
    base = recommend(model, None, users, k=20, exclude=pairs)      # the model's own item_embeddings
    assert not model.training
    for other in (recommend(model, None, users, k=20, exclude=pairs, table=world["table"]),
                  recommend(model, None, users, k=20, exclude=(world["indptr"], world["excl"]))):
        assert np.array_equal(other[0], base[0]) and np.array_equal(other[1].view(np.uint32), base[1].view(np.uint32))
    # another batch size: the per-user half Pu of layer 0 is a dense product over the batch's rows, whose order of sums is the BLAS's and may
    # differ with the row count, so the bits may; the j-th best score of a user moves by no more than any score does
    small = recommend(model, None, users, k=20, exclude=pairs, batch_users=2)
    live = base[0] >= 0
    assert np.array_equal(small[0] >= 0, live) and np.abs(small[1][live].astype(np.float64) - base[1][live]).max() <= world["tol"]
    with pytest.raises(ValueError, match="item table"):
        recommend(model, None, users, k=3, table=torch.zeros(N_ITEMS, 8, device="cuda"))
    with pytest.raises(ValueError, match="users"):
        recommend(model, None, np.array([USER_NUM]), k=3)


def test_a_model_with_dropout_is_scored_without_masks(world):
    from pmgt_amd.dcn import DCN
    from pmgt_amd.recommend import recommend
    model, users, pairs, head = world["model"], world["users"][:9], world["pairs"], world["head"]
    dropped = DCN(USER_NUM, N_ITEMS, *head[:3], emb_dropout=0.2, dropout=0.3, use_layer_norm=head[3], layer_norm_eps=EPS).cuda()
    dropped.load_state_dict(model.state_dict())
    dropped.train()
    got, want = recommend(dropped, None, users, k=5, exclude=pairs), recommend(model, None, users, k=5, exclude=pairs)
    assert dropped.training and np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))


def test_a_nan_in_the_item_rows_raises(world):
    from pmgt_amd.recommend import recommend
    model, users = world["model"], world["users"]
    table = world["table"].clone()
    table[4, 1] = float("nan")
    for impl in ("device", "host"):
        with pytest.raises(ValueError, match=f"of {len(users)} users have a NaN score"):
            recommend(model, None, users, k=3, impl=impl, table=table)
    # excluded for everyone who is asked: no NaN among the eligible scores, no error
    recommend(model, None, users[2:4], k=3, exclude=[(int(u), 4) for u in users[2:4]], table=table)


def test_the_loop_never_syncs(world, monkeypatch):
    from pmgt_amd.dcn_train import _flat_of
    from pmgt_amd.recommend import DcnScorer, TopkRows, recommend
    model, users, table = world["model"], world["users"], world["table"]
    base = recommend(model, None, users, k=20, exclude=world["pairs"], table=table, batch_users=4)      # warm
    calls = []
    real = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    again = recommend(model, None, users, k=20, exclude=world["pairs"], table=table, batch_users=4)
    assert not calls and np.array_equal(again[0], base[0])
    # the body of the loop under the sync detector: a copy to the host or a wait would raise
    dev = model.output_layer.weight.device
    with torch.no_grad():
        scorer = DcnScorer(_flat_of(model, dropout_ok=True), table, model.layer_norm_eps)
        picker = TopkRows(dev, 4, N_ITEMS, 20, world["indptr"], world["excl"], model.user_num)
        ud = torch.from_numpy(users).to(dev)
        work = torch.empty(4, N_ITEMS, device=dev)
        out = (torch.empty(len(users), 20, dtype=torch.int32, device=dev), torch.empty(len(users), 20, device=dev),
               torch.empty(len(users), dtype=torch.int32, device=dev))
        real()
        before = torch.cuda.get_sync_debug_mode()
        torch.cuda.set_sync_debug_mode("error")
        try:
            for lo in range(0, len(users), 4):
                hi = min(lo + 4, len(users))
                scorer.score(ud[lo:hi], out=work)
                picker.select(work[: hi - lo], ud[lo:hi], out=tuple(t[lo:hi] for t in out))
        finally:
            torch.cuda.set_sync_debug_mode(before)
    assert np.array_equal(out[0].cpu().numpy().astype(np.int64), base[0])
