"""recommend() end to end on the two PMGT_NCF golden cases (built as tests/test_evaluate_ranking_gpu.py builds them): the device path against
the host path.  The two sum a logit in different orders, so the comparison does not ask for equal bits: with s_h the host's full score rows
and tol = 4 max(max|s_h - o64|, 2^-22 max|o64|) (the bound of tests/test_ncf_score_gpu.py with model.head as the fp32 formula and
ncf_head_host on the model's state_dict as o64), per user
  (a) the returned items are unique, in range, never excluded, and -1 exactly where the host pads;
  (b) the returned scores are non-increasing, equal-score neighbours in index order;
  (c) |score_dev - s_h[item]| <= tol;
  (d) every returned item has s_h[item] >= (k-th best eligible s_h) - 2 tol: the right set up to near-ties."""
import numpy as np
import pytest
import torch

from tests.test_evaluate_ranking_gpu import build

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["ncf_mlp", "ncf_neumf"])
def world(request):
    from pmgt_amd.recommend import exclusion_csr, host_scores, ncf_head_host
    from pmgt_amd.trainer import encode_catalogue
    w = build(request.param)
    model, n_users, n_items = w["model"], w["case"]["users"], w["case"]["n_nodes"]
    rng = np.random.default_rng(11)
    # a synthetic interaction list: user 0 has nothing excluded, user 1 every item but three, the others 1 .. 24 items
    pairs = [(1, int(i)) for i in rng.permutation(n_items)[3:]]
    pairs += [(u, int(i)) for u in range(2, n_users) for i in rng.choice(n_items, size=int(rng.integers(1, 25)), replace=False)]
    users = np.concatenate([np.arange(n_users), [1, 0, n_users - 1]])      # users come twice
    model.eval()
    table = encode_catalogue(model, w["sampler"])
    s_h = host_scores(model, table, users)
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items() if not k.startswith(("bert.", "feat_embeddings."))}
    o64 = ncf_head_host(sd, users, table.cpu().numpy(), np.float64)
    tol = 4 * max(np.abs(s_h - o64).max(), 2.0 ** -22 * np.abs(o64).max())
    indptr, excl = exclusion_csr(pairs, n_users, n_items)
    w.update(pairs=pairs, users=users, table=table, s_h=s_h, tol=tol, indptr=indptr, excl=excl, n_items=n_items)
    return w


@pytest.mark.parametrize("k", [1, 20, "above the item count"])
def test_device_path_against_host_path(world, k):
    from pmgt_amd.recommend import recommend
    model, sampler, users, s_h, tol, n_items = (world[x] for x in ("model", "sampler", "users", "s_h", "tol", "n_items"))
    k = n_items + 5 if isinstance(k, str) else k
    model.train()
    it_d, sc_d = recommend(model, sampler, users, k=k, exclude=world["pairs"], impl="device")
    it_h, sc_h = recommend(model, sampler, users, k=k, exclude=world["pairs"], impl="host")
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
    print(f"k = {k}: {exact} of {len(users)} users get exactly the host's item list (tol {tol:.3e})")
    assert (it_d[0] >= 0).sum() == min(k, n_items) and (it_d[1] >= 0).sum() == min(k, 3)      # nothing excluded / all but three


def test_batching_table_reuse_and_mode(world):
    from pmgt_amd.recommend import recommend
    model, sampler, users, pairs = world["model"], world["sampler"], world["users"], world["pairs"]
    model.eval()
    base = recommend(model, sampler, users, k=20, exclude=pairs)
    assert not model.training
    for other in (recommend(model, sampler, users, k=20, exclude=pairs, batch_users=2),
                  recommend(model, sampler, users, k=20, exclude=pairs, table=world["table"]),
                  recommend(model, sampler, users, k=20, exclude=(world["indptr"], world["excl"]))):
        assert np.array_equal(other[0], base[0]) and np.array_equal(other[1].view(np.uint32), base[1].view(np.uint32))
    free = recommend(model, sampler, users[:3], k=5, table=world["table"])
    assert (free[0] >= 0).all()


def test_a_nan_in_the_table_raises(world):
    from pmgt_amd.recommend import recommend
    model, sampler, users = world["model"], world["sampler"], world["users"]
    table = world["table"].clone()
    table[4, 1] = float("nan")
    for impl in ("device", "host"):
        with pytest.raises(ValueError, match=f"of {len(users)} users have a NaN score"):
            recommend(model, sampler, users, k=3, impl=impl, table=table)
    # excluded for everyone who is asked: no NaN among the eligible scores, no error
    recommend(model, sampler, users[2:4], k=3, exclude=[(int(u), 4) for u in users[2:4]], table=table)


def test_the_loop_never_syncs(world, monkeypatch):
    from pmgt_amd.recommend import NcfScorer, TopkRows, recommend
    model, sampler, users = world["model"], world["sampler"], world["users"]
    base = recommend(model, sampler, users, k=20, exclude=world["pairs"], table=world["table"], batch_users=4)      # warm
    calls = []
    real = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    again = recommend(model, sampler, users, k=20, exclude=world["pairs"], table=world["table"], batch_users=4)
    assert not calls and np.array_equal(again[0], base[0])
    # the body of the loop under the sync detector: a copy to the host or a wait would raise
    dev = model.engine.device
    sd = {k: v for k, v in model.state_dict().items() if not k.startswith(("bert.", "feat_embeddings."))}
    with torch.no_grad():
        scorer = NcfScorer(sd, world["table"])
        picker = TopkRows(dev, 4, world["n_items"], 20, world["indptr"], world["excl"], model.user_num)
        ud = torch.from_numpy(users).to(dev)
        work = torch.empty(4, world["n_items"], device=dev)
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
