"""evaluate_catalogue() end to end on a PMGT_NCF golden case, the stand-alone NCF class (LayerNorm NeuMF-end, and kind GMF) and the two DCN
shapes of tests/test_recommend_dcn_gpu.py (the VALU scorer and the MFMA tile at its widest), at the sizes of the recommend tests:
  (a) impl="device" equals the numpy yardstick (heldout_ranks_host, catalogue_metrics_host) applied to the device scorer's OWN score rows,
      bit for bit, for batch_users in {1, 7, all} (the rows are scored in the same batches: the per-user half of layer 0 is a dense
      product over the batch's rows, whose order of sums is the BLAS's);
  (b) against impl="host", per held-out pair, |rank_dev - rank_host| <= the number of OTHER eligible items whose host score lies within
      tau of the item's host score, tau = 4 max(max|s_h - o64|, 2^-22 max|o64|): the bound the recommend tests of each class hold the
      scorer to at this shape; no other tolerance;
  (c) the places rank - 1 are those of recommend(k=20, impl="device") for every held-out item it returns;
  (d) a table passed as table= is read in place, and the caller's train / eval mode is restored."""
import numpy as np
import pytest
import torch

from pmgt_amd.catalogue_eval import catalogue_metrics_host, evaluate_catalogue, heldout_csr, heldout_ranks_host
from pmgt_amd.recommend import DcnScorer, NcfModelScorer, NcfScorer, dcn_host_scores, exclusion_csr, host_scores, recommend

pytestmark = pytest.mark.gpu

KS = (5, 10, 20)


def interactions(user_num, n_items, seed=11):
    """Every user but the last two is evaluated: 1 .. 14 held-out items and 1 .. 14 excluded ones, disjoint; user 1 keeps three eligible
    items, one of them held out; the last user has exclusions and nothing held out."""
    rng = np.random.default_rng(seed)
    held, excl = [], []
    for u in range(user_num - 2):
        if u == 1:
            left = rng.permutation(n_items)
            held += [(1, int(left[0]))]
            excl += [(1, int(i)) for i in left[3:]]
            continue
        drawn = rng.choice(n_items, size=min(int(rng.integers(2, 29)), n_items // 2), replace=False)
        cut = int(rng.integers(1, len(drawn)))
        held += [(u, int(i)) for i in drawn[:cut]]
        excl += [(u, int(i)) for i in drawn[cut:]]
    excl += [(user_num - 1, 0), (user_num - 1, min(7, n_items - 1))]
    return held, excl


@pytest.fixture(scope="module", params=["pmgt-neumf", "ncf-ln", "ncf-gmf", "dcn", "dcn-mfma"])
def world(request):
    kind = request.param
    sampler = None
    if kind == "pmgt-neumf":
        from pmgt_amd.recommend import ncf_head_host
        from pmgt_amd.trainer import encode_catalogue
        from tests.test_evaluate_ranking_gpu import build
        w = build("ncf_neumf")
        model, sampler, user_num, n_items = w["model"], w["sampler"], w["case"]["users"], w["case"]["n_nodes"]
        model.eval()
        table = encode_catalogue(model, sampler)
        sd = {k: v for k, v in model.state_dict().items() if not k.startswith(("bert.", "feat_embeddings."))}
        scorer = lambda t: NcfScorer(sd, t)
        host = lambda us, t: host_scores(model, t, us)
        o64 = lambda us: ncf_head_host({k: v.detach().cpu() for k, v in sd.items()}, us, table.cpu().numpy(), np.float64)
    elif kind.startswith("dcn"):
        from pmgt_amd.dcn_head import dcn_scores_host
        from pmgt_amd.dcn_train import _flat_of
        from tests.dcn_score_util import EPS, ITEMS, USER_NUM, world as scored
        from tests.dcn_util import torch_model
        head = (16, 1, 4, True) if kind == "dcn" else (64, 2, 6, True)
        wts = scored(head)["w"]
        model, user_num, n_items = torch_model({k: np.array(v) for k, v in wts.items()}, head, device="cuda"), USER_NUM, ITEMS[-1]
        table = torch.cat([torch.zeros(1, head[0] << head[1], device="cuda"), model.item_embeddings.weight.detach()])[1:]
        scorer = lambda t: DcnScorer(_flat_of(model, dropout_ok=True), t, model.layer_norm_eps)
        host = lambda us, t: dcn_host_scores(model, t, us)
        o64 = lambda us: dcn_scores_host(wts, us, None, np.float64, EPS)
    else:
        from pmgt_amd.ncf_model import ncf_model_scores_host
        from tests.ncf_model_score_util import EPS, ITEMS, USER_NUM, world as scored
        from tests.ncf_model_util import torch_model
        head = (64, 2, "NeuMF-end", True) if kind == "ncf-ln" else (8, 2, "GMF", False)
        wts = scored(head)["w"]
        model, user_num, n_items = torch_model({k: np.array(v) for k, v in wts.items()}, head, device="cuda"), USER_NUM, ITEMS[-1]
        table = None
        if head[2] != "GMF":                                 # a view of another buffer holding the model's item rows
            table = torch.cat([torch.zeros(1, 2 * head[0], device="cuda"), model.embed_item_MLP.weight.detach()])[1:]
        scorer = lambda t: NcfModelScorer(model.state_dict(), t, model.model, model.layer_norm_eps)
        host = lambda us, t: host_scores(model, torch.empty(n_items, 0, device="cuda") if t is None else t, us)
        o64 = lambda us: ncf_model_scores_host(wts, us, None, np.float64, EPS, head[2])
    held, excl = interactions(user_num, n_items)
    h_csr, e_csr = heldout_csr(held, user_num, n_items), exclusion_csr(excl, user_num, n_items)
    users = np.nonzero(np.diff(h_csr[0]) > 0)[0].astype(np.int64)
    model.eval()
    s_h = host(users, table)
    ref = o64(users)
    tol = 4 * max(np.abs(s_h - ref).max(), 2.0 ** -22 * np.abs(ref).max())
    return dict(kind=kind, model=model, sampler=sampler, table=table, user_num=user_num, n_items=n_items, held=held, excl=excl, h_csr=h_csr,
                e_csr=e_csr, users=users, s_h=s_h, tol=tol, scorer=scorer)


def own_scores(world, table, batch):
    """The device scorer's score rows of the evaluated users, scored in batches of `batch` as evaluate_catalogue scores them"""
    with torch.no_grad():
        sc = world["scorer"](table)
        ud = torch.from_numpy(world["users"]).cuda()
        return np.concatenate([sc.score(ud[lo: lo + batch]).cpu().numpy() for lo in range(0, len(ud), batch)])


@pytest.mark.parametrize("batch", [1, 7, None])
def test_device_equals_the_yardstick_on_the_scorers_own_rows(world, batch):
    model, users, h_csr = world["model"], world["users"], world["h_csr"]
    model.train()
    result, pu = evaluate_catalogue(model, world["sampler"], world["held"] + world["held"][:3], exclude=world["excl"], ks=KS, batch_users=batch,
                                    table=world["table"], per_user=True)
    assert model.training                                     # the mode the caller had is restored
    s_d = own_scores(world, world["table"], batch or len(users))
    ranks, flags = heldout_ranks_host(s_d, users, h_csr, world["e_csr"])
    m = catalogue_metrics_host(ranks, h_csr[0], KS)
    assert not flags.any() and np.array_equal(pu["ranks"], ranks) and np.array_equal(pu["users"], users)
    assert np.array_equal(pu["indptr"], h_csr[0]) and np.array_equal(pu["items"], h_csr[1]) and np.array_equal(pu["n_pos"], m["n_pos"])
    U = len(users)
    for k in KS:
        for name, key in (("ndcg", "n"), ("recall", "r"), ("hit", "hr")):
            assert pu[name][k].tobytes() == m[name][k].tobytes(), (name, k)
            assert result[f"{key}{k}"] == m["sums"][name][k] / U, (name, k)
    assert pu["rr"].tobytes() == m["rr"].tobytes() and result["mrr"] == m["sums"]["rr"] / U
    assert result["users"] == U and result["pairs"] == len(world["held"])
    assert ranks[h_csr[0][1]] <= 3                            # user 1: three eligible items


def test_against_the_host_path_within_the_scorers_bound(world):
    model, users, h_csr, e_csr, s_h, tol = (world[x] for x in ("model", "users", "h_csr", "e_csr", "s_h", "tol"))
    model.eval()
    kw = dict(exclude=world["e_csr"], ks=KS, table=world["table"], per_user=True)
    res_d, pu_d = evaluate_catalogue(model, world["sampler"], h_csr, impl="device", **kw)
    res_h, pu_h = evaluate_catalogue(model, world["sampler"], h_csr, impl="host", **kw)
    assert not model.training
    ranks_h, _ = heldout_ranks_host(s_h, users, h_csr, e_csr)
    assert np.array_equal(pu_h["ranks"], ranks_h)
    moved = 0
    for r, u in enumerate(users):
        elig = np.ones(world["n_items"], dtype=bool)
        elig[e_csr[1][e_csr[0][u]: e_csr[0][u + 1]]] = False
        for h in range(h_csr[0][u], h_csr[0][u + 1]):
            p = h_csr[1][h]
            near = int(np.count_nonzero(elig & (np.abs(s_h[r] - s_h[r, p]) <= tol))) - 1      # the others
            assert abs(int(pu_d["ranks"][h]) - int(ranks_h[h])) <= near, (u, p, pu_d["ranks"][h], ranks_h[h], near)
            moved += pu_d["ranks"][h] != ranks_h[h]
    print(f"{world['kind']}: {moved} of {len(ranks_h)} ranks differ between device and host (tau {tol:.3e}); device {res_d}; host {res_h}")


def test_places_agree_with_recommend(world):
    model, users, h_csr = world["model"], world["users"], world["h_csr"]
    model.eval()
    _, pu = evaluate_catalogue(model, world["sampler"], h_csr, exclude=world["e_csr"], ks=KS, table=world["table"], per_user=True)
    items, _ = recommend(model, world["sampler"], users, k=20, exclude=world["e_csr"], impl="device", table=world["table"])
    seen = 0
    for r, u in enumerate(users):
        for h in range(h_csr[0][u], h_csr[0][u + 1]):
            where = np.nonzero(items[r] == h_csr[1][h])[0]
            if pu["ranks"][h] <= 20:
                assert where.tolist() == [pu["ranks"][h] - 1]
                seen += 1
            else:
                assert len(where) == 0
    assert seen > 0


def test_the_table_is_read_in_place(world):
    model = world["model"]
    if world["table"] is None:                               # kind GMF reads no item table and says so
        with pytest.raises(ValueError, match="evaluate_catalogue: kind 'GMF' reads no item table"):
            evaluate_catalogue(model, None, world["h_csr"], table=torch.zeros(world["n_items"], 16, device="cuda"))
        return
    table = world["table"].clone()
    before = table.clone()
    base = evaluate_catalogue(model, world["sampler"], world["h_csr"], exclude=world["e_csr"], ks=KS, table=world["table"])
    assert evaluate_catalogue(model, world["sampler"], world["h_csr"], exclude=world["e_csr"], ks=KS, table=table) == base
    assert torch.equal(table, before)
    # the same buffer with other rows in it: the result follows the buffer
    table.copy_(before.flip(0))
    _, pu = evaluate_catalogue(model, world["sampler"], world["h_csr"], exclude=world["e_csr"], ks=KS, table=table, per_user=True)
    ranks, _ = heldout_ranks_host(own_scores(world, table, len(world["users"])), world["users"], world["h_csr"], world["e_csr"])
    assert np.array_equal(pu["ranks"], ranks) and torch.equal(table, before.flip(0))


def test_refusals_on_the_device_path(world):
    model, held, excl = world["model"], world["held"], world["excl"]
    with pytest.raises(ValueError, match=f"2 of {len(held)} held-out pairs are also excluded"):
        evaluate_catalogue(model, world["sampler"], held, exclude=excl + held[:2], table=world["table"])
    with pytest.raises(ValueError, match="the held-out set is empty"):
        evaluate_catalogue(model, world["sampler"], [], table=world["table"])
    with pytest.raises(ValueError, match="heldout: users in"):
        evaluate_catalogue(model, world["sampler"], [(world["user_num"], 0)], table=world["table"])
    if world["table"] is not None:
        table = world["table"].clone()
        table[4, 1] = float("nan")
        few = [(0, 1), (2, 3), (3, 5)]
        for impl in ("device", "host"):
            with pytest.raises(ValueError, match="2 of 3 users have a NaN score among their eligible items"):
                evaluate_catalogue(model, world["sampler"], few, exclude=[(2, 4)], impl=impl, table=table)
        evaluate_catalogue(model, world["sampler"], few, exclude=[(0, 4), (2, 4), (3, 4)], table=table)      # excluded for all: no error


def test_the_loop_never_syncs(world, monkeypatch):
    """evaluate_catalogue ITSELF with the sync detector on "error" from the first scorer call to the copy of the header: a copy to the host,
    an .item() or a wait inside its loop, or in the reduce behind it, raises.  (The uploads before the loop are synchronous copies and stay
    outside; the header's copy is the one the function is allowed.)"""
    from pmgt_amd import catalogue_eval
    from pmgt_amd.recommend import ModelDispatch
    model, users, h_csr, e_csr = world["model"], world["users"], world["h_csr"], world["e_csr"]
    kw = dict(exclude=e_csr, ks=KS, table=world["table"], batch_users=4)
    base = evaluate_catalogue(model, world["sampler"], h_csr, **kw)      # warm
    calls = []
    real = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    before = torch.cuda.get_sync_debug_mode()
    seen = dict(score=0, rank=0, copies=0)
    make_scorer, rank, statistic = ModelDispatch.scorer, catalogue_eval.HeldoutRanks.rank, catalogue_eval.CatalogueMetrics.statistic

    def guarded_scorer(self):
        scorer = make_scorer(self)
        score = scorer.score

        def guarded_score(*a, **k):
            if not seen["score"]:
                real()
                torch.cuda.set_sync_debug_mode("error")      # from here on
            seen["score"] += 1
            return score(*a, **k)
        scorer.score = guarded_score
        return scorer

    def counted_rank(self, *a, **k):
        assert torch.cuda.get_sync_debug_mode() == 2          # "error": the loop runs under the detector
        seen["rank"] += 1
        return rank(self, *a, **k)

    def allowed_copy(self):
        torch.cuda.set_sync_debug_mode(before)                # up to here: the one small copy out
        seen["copies"] += 1
        return statistic(self)
    monkeypatch.setattr(ModelDispatch, "scorer", guarded_scorer)
    monkeypatch.setattr(catalogue_eval.HeldoutRanks, "rank", counted_rank)
    monkeypatch.setattr(catalogue_eval.CatalogueMetrics, "statistic", allowed_copy)
    try:
        again = evaluate_catalogue(model, world["sampler"], h_csr, **kw)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    batches = -(-len(users) // 4)
    assert again == base and not calls and seen == dict(score=batches, rank=batches, copies=1)
