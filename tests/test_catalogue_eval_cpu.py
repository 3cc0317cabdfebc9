"""The numpy yardstick of the whole-catalogue evaluation (heldout_ranks_host, catalogue_metrics_host) against the reference's recorded
get_ndcg / get_recall on whole-catalogue lists, against topk_host, on ties and NaNs, and evaluate_catalogue(impl="host") on CPU models."""
import os
import re

import numpy as np
import pytest

from pmgt_amd import _build, _lib
from pmgt_amd.catalogue_eval import (catalogue_metrics_host, evaluate_catalogue, heldout_csr, heldout_ranks_host, summarize_catalogue,
                                     tree_sum_host)
from pmgt_amd.recommend import dcn_host_scores, exclusion_csr, host_scores, topk_host

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "catalogue_eval_48x300.npz")
NAN, GONE = _lib.TOPK_FLAG_NAN, _lib.RANK_HELDOUT_FLAG_EXCLUDED


@pytest.fixture(scope="module")
def golden():
    g = dict(np.load(GOLDEN))
    g["users"] = np.arange(len(g["scores"]))
    g["held"], g["excl"] = (g["held_indptr"], g["held_items"]), (g["excl_indptr"], g["excl_items"])
    g["ranks"], g["flags"] = heldout_ranks_host(g["scores"], g["users"], g["held"], g["excl"])
    for v in g.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return g


def csr(lists):
    return (np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int64),
            np.concatenate([np.asarray(l, dtype=np.int32) for l in lists] + [np.zeros(0, np.int32)]).astype(np.int32))


def positions_agree(x, users, held, excl, ranks, ks):
    """rank <= k exactly when the item sits at place rank - 1 of topk_host(k)"""
    for k in ks:
        items, _, _ = topk_host(x, k, excl[0] if excl else None, excl[1] if excl else None, users)
        for r, u in enumerate(users):
            for h in range(held[0][u], held[0][u + 1]):
                p, rank = held[1][h], ranks[h]
                where = np.nonzero(items[r] == p)[0]
                if rank == 0:
                    assert len(where) == 0                   # excluded: in no list
                elif rank <= k:
                    assert where.tolist() == [rank - 1], (k, u, p, rank)
                else:
                    assert len(where) == 0, (k, u, p, rank)


def test_fixture_is_what_the_generator_describes(golden):
    g = golden
    assert g["scores"].shape == (48, 300) and g["scores"].dtype == np.float32 and g["predictions"].shape == (48, 100)
    n_excl, n_held = np.diff(g["excl_indptr"]), np.diff(g["held_indptr"])
    assert n_excl.min() == 0 and n_excl.max() == 40 and n_held.min() == 1 and n_held.max() > 20
    for u in range(48):
        e = set(g["excl_items"][g["excl_indptr"][u]: g["excl_indptr"][u + 1]].tolist())
        h = set(g["held_items"][g["held_indptr"][u]: g["held_indptr"][u + 1]].tolist())
        assert not e & h and not e & set(g["predictions"][u].tolist())
    # the reference's list is the project's order on tie-free rows
    items, _, _ = topk_host(g["scores"], 100, *g["excl"], g["users"])
    assert np.array_equal(items, g["predictions"])


def test_reference_metrics_bit_for_bit(golden):
    g = golden
    assert not g["flags"].any() and (g["ranks"] >= 1).all()
    m = catalogue_metrics_host(g["ranks"], g["held_indptr"], (10, 20))
    assert np.array_equal(m["users"], g["users"]) and np.array_equal(m["n_pos"], np.diff(g["held_indptr"]))
    U = 48
    for k in (10, 20):
        assert np.array_equal(m["ndcg"][k], g[f"n{k}_user"]) and np.array_equal(m["recall"][k], g[f"r{k}_user"]), k
        for got, want in ((m["sums"]["ndcg"][k] / U, float(g[f"n{k}"])), (m["sums"]["recall"][k] / U, float(g[f"r{k}"]))):
            assert abs(got - want) <= U * 2.0 ** -52 * abs(want), (k, got, want)
    out = summarize_catalogue(m["sums"], U, len(g["held_items"]), (10, 20))
    assert set(out) == {"n10", "n20", "r10", "r20", "hr10", "hr20", "mrr", "users", "pairs"} and out["users"] == 48
    assert out["pairs"] == len(g["held_items"]) and 0 < out["mrr"] <= 1 and out["hr10"] <= out["hr20"] <= 1
    # hit and rr from the reference's list: the first place of a held-out item
    for u in range(U):
        h = g["held_items"][g["held_indptr"][u]: g["held_indptr"][u + 1]]
        first = np.nonzero(np.isin(g["predictions"][u], h))[0]
        if len(first) and first[0] < 20:
            assert m["rr"][u] == 1.0 / (first[0] + 1) and m["hit"][20][u] == 1.0 and m["hit"][10][u] == float(first[0] < 10)
        else:
            assert m["hit"][20][u] == 0.0


def test_ranks_are_the_places_of_topk_host(golden):
    g = golden
    n_elig = 300 - int(np.diff(g["excl_indptr"]).max())
    positions_agree(g["scores"], g["users"], g["held"], g["excl"], g["ranks"], (1, 20, n_elig))
    # k = the eligible count of every user separately: the whole list
    for u in (0, 7, 47):
        k = 300 - int(np.diff(g["excl_indptr"])[u])
        positions_agree(g["scores"][u:u + 1], g["users"][u:u + 1], g["held"], g["excl"], g["ranks"], (k,))


def tie_rows(n_items=70):
    rng = np.random.default_rng(3)
    inf = np.float32(np.inf)
    rows = [rng.integers(0, 3, n_items).astype(np.float32),                    # three values
            np.full(n_items, 0.25, dtype=np.float32),                           # all equal
            np.where(rng.integers(0, 2, n_items) == 1, np.float32(0.0), np.float32(-0.0)).astype(np.float32),      # +0.0 against -0.0
            rng.choice(np.array([-inf, -1, 0, 1, inf], dtype=np.float32), n_items),      # +-inf
            np.where(np.arange(n_items) % 3 == 0, -inf, rng.standard_normal(n_items)).astype(np.float32)]      # -inf on eligible items
    return np.stack(rows)


def test_ties_and_infinities():
    x = tie_rows()
    n, n_items = x.shape
    rng = np.random.default_rng(4)
    users = np.arange(n)
    excl_lists = [np.concatenate([e, e[:2]]) for e in (rng.choice(n_items, 9, replace=False) for _ in range(n))]      # with duplicates
    excl_lists[1] = np.zeros(0, np.int64)                    # a user with no exclusions
    held_pairs = [(u, int(p)) for u in range(n) for p in np.setdiff1d(np.arange(n_items), excl_lists[u])[::5]]
    held = heldout_csr(held_pairs + held_pairs[:4], n, n_items)      # duplicates are dropped
    assert len(held[1]) == len(held_pairs)
    excl = csr(excl_lists)
    ranks, flags = heldout_ranks_host(x, users, held, excl)
    assert not flags.any() and (ranks >= 1).all()
    positions_agree(x, users, held, excl, ranks, (1, 20, n_items))
    # all equal, nothing excluded: place = item index + 1
    assert np.array_equal(ranks[held[0][1]: held[0][2]], held[1][held[0][1]: held[0][2]] + 1)
    # the definition, counted one by one
    from pmgt_amd.evaluation import score_key
    for u in range(n):
        key = score_key(x[u]).astype(np.int64)
        elig = np.ones(n_items, bool)
        elig[excl_lists[u]] = False
        for h in range(held[0][u], held[0][u + 1]):
            p = held[1][h]
            above = sum(1 for j in range(n_items) if elig[j] and j != p and (key[j] > key[p] or (key[j] == key[p] and j < p)))
            assert ranks[h] == 1 + above


def test_nan_excluded_and_single_eligible():
    n_items = 40
    x = np.linspace(-1, 1, 4 * n_items, dtype=np.float32).reshape(4, n_items).copy()
    x[0, 17] = x[1, 17] = np.nan
    users = np.arange(4)
    # user 0: the NaN is eligible; user 1: it is excluded; user 2: a held-out item is excluded; user 3: everything but item 5 is excluded
    excl = csr([[], [17], [3, 8], [j for j in range(n_items) if j != 5]])
    held = csr([[2, 17], [2], [3, 4], [5]])
    ranks, flags = heldout_ranks_host(x, users, held, excl)
    assert flags.tolist() == [NAN, 0, GONE, 0]
    assert ranks[1] == 1 and ranks[0] == 1 + (n_items - 2 - 1)      # the NaN first; item 2 behind it and the 37 larger scores
    assert ranks[2] == n_items - 3                                   # user 1: the NaN is excluded, item 2 behind the 36 other larger scores
    assert ranks[3] == 0 and ranks[4] == n_items - 4 - 1            # item 3 excluded: no rank; item 4: 35 larger scores, one of them excluded
    assert ranks[5] == 1
    positions_agree(x, users, held, excl, ranks, (1, 20, n_items))
    m = catalogue_metrics_host(ranks, held[0], (1, 10))
    assert m["n_pos"].tolist() == [2, 1, 2, 1] and m["rr"][3] == 1.0 and m["hit"][1].tolist() == [1.0, 0.0, 0.0, 1.0]
    assert m["recall"][10][2] == 0.0 and m["ndcg"][10][3] == 1.0 and m["rr"][2] == 1.0 / ranks[4]
    # a user without a held-out item: no row of results, its row of scores is never looked at
    r2, f2 = heldout_ranks_host(x, np.array([0, 1, 2, 3]), csr([[2], [], [], [5]]), excl)
    assert r2.tolist() == [ranks[0], 1] and f2.tolist() == [NAN, 0, 0, 0]


def test_tree_sum_is_a_sum_in_a_fixed_order():
    rng = np.random.default_rng(0)
    for n in (1, 5, 256, 257, 1000):
        v = rng.random(n)
        assert abs(tree_sum_host(v) - v.sum()) <= n * 2.0 ** -52 * v.sum()
    assert tree_sum_host([0.5]) == 0.5 and tree_sum_host(np.ones(700)) == 700.0


def test_refusals():
    x = np.zeros((2, 5), dtype=np.float32)
    with pytest.raises(ValueError, match=r"must be \[n, I\]"):
        heldout_ranks_host(np.zeros(5, np.float32), [0], csr([[1]]))
    with pytest.raises(ValueError, match=r"users .* must be \[n = 2\]"):
        heldout_ranks_host(x, [0], csr([[1], [2]]))
    with pytest.raises(ValueError, match="non-decreasing from 0 to len"):
        catalogue_metrics_host([1, 2], [0, 3], (1,))
    with pytest.raises(ValueError, match="no held-out item"):
        catalogue_metrics_host([], [0, 0, 0], (1,))
    for ks in ((), (0,), (20, 10), (1, 2, 3, 4, 5), (1025,)):
        with pytest.raises(ValueError, match="ks="):
            catalogue_metrics_host([1], [0, 1], ks)
    with pytest.raises(ValueError, match=r"heldout: users in \[\d+, \d+\] outside"):
        heldout_csr([(9, 0)], 3, 5)
    with pytest.raises(ValueError, match=r"heldout: held-out items in \[\d+, \d+\] outside"):
        heldout_csr([(0, 5)], 3, 5)
    with pytest.raises(ValueError, match=r"heldout: expected \(user, item\) integer pairs"):
        heldout_csr(np.zeros((2, 3), dtype=np.int64), 3, 5)
    with pytest.raises(ValueError, match="heldout: indptr must be non-decreasing"):
        heldout_csr((np.array([0, 2, 1, 1]), np.array([0], dtype=np.int32)), 3, 5)
    indptr, items = heldout_csr((np.array([0, 3, 3, 4]), np.array([4, 1, 4, 0], dtype=np.int32)), 3, 5)      # a ready CSR: sorted, unique
    assert indptr.tolist() == [0, 2, 2, 3] and items.tolist() == [1, 4, 0] and items.dtype == np.int32


def test_the_entries_are_declared_bound_and_built():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "pmgt_capi.h")).read()
    for sym in ("pmgt_rank_heldout", "pmgt_rank_heldout_reduce"):
        assert re.search(r"\b" + sym + r"\(", hdr) and sym in _lib.HIP_SYMBOLS, sym
    assert any(p.endswith(os.path.join("ops", "catalogue_rank.hip")) for p in _build.OPS_SOURCES)
    assert "#define PMGT_RANK_HELDOUT_CHUNK 1024" in hdr and _lib.RANK_HELDOUT_CHUNK == 1024
    assert "#define PMGT_RANK_HELDOUT_FLAG_EXCLUDED 4u" in hdr and GONE == 4
    import pmgt_amd
    for name in ("evaluate_catalogue", "heldout_ranks_host", "catalogue_metrics_host", "HeldoutRanks", "CatalogueMetrics"):
        assert name in pmgt_amd.__all__ and hasattr(pmgt_amd, name)


# ---- evaluate_catalogue(impl="host") on CPU models ----------------------------------------------------------------------------------------------
def interactions(user_num, n_items, seed=11):
    rng = np.random.default_rng(seed)
    excl, held = [], []
    for u in range(0, user_num, 2):                          # every second user is evaluated
        drawn = rng.choice(n_items, size=int(rng.integers(2, 30)), replace=False)
        cut = int(rng.integers(1, len(drawn)))
        held += [(u, int(i)) for i in drawn[:cut]]
        excl += [(u, int(i)) for i in drawn[cut:]]
    excl += [(1, 0), (1, 7)]                                  # a user with exclusions and nothing held out
    return held, excl


def cpu_model(kind):
    if kind == "dcn":
        from tests.dcn_score_util import ITEMS, USER_NUM, world
        from tests.dcn_util import torch_model
        head = (16, 1, 4, True)
        return torch_model({k: np.array(v) for k, v in world(head)["w"].items()}, head), USER_NUM, ITEMS[-1]
    from tests.ncf_model_score_util import ITEMS, USER_NUM, world
    from tests.ncf_model_util import torch_model
    head = (8, 2, "NeuMF-end", True) if kind == "ncf" else (8, 2, "GMF", False)
    return torch_model({k: np.array(v) for k, v in world(head)["w"].items()}, head), USER_NUM, ITEMS[-1]


@pytest.mark.parametrize("kind", ["ncf", "gmf", "dcn"])
def test_evaluate_catalogue_host_on_cpu_models(kind):
    import torch
    model, user_num, n_items = cpu_model(kind)
    held, excl = interactions(user_num, n_items)
    model.train()
    result, pu = evaluate_catalogue(model, None, held + held[:5], exclude=excl, ks=(5, 10, 20), impl="host", per_user=True)
    assert model.training
    assert result == evaluate_catalogue(model, None, held, exclude=exclusion_csr(excl, user_num, n_items), ks=(5, 10, 20), impl="host")
    users = np.arange(0, user_num, 2)
    assert np.array_equal(pu["users"], users) and result["users"] == len(users) and result["pairs"] == len(held)
    model.eval()
    if kind == "dcn":
        s = dcn_host_scores(model, None, users)
    else:
        table = torch.empty(n_items, 0) if kind == "gmf" else model.embed_item_MLP.weight.detach()
        s = host_scores(model, table, users)
    h_csr, e_csr = heldout_csr(held, user_num, n_items), exclusion_csr(excl, user_num, n_items)
    ranks, flags = heldout_ranks_host(s, users, h_csr, e_csr)
    m = catalogue_metrics_host(ranks, h_csr[0], (5, 10, 20))
    assert not flags.any() and np.array_equal(pu["ranks"], ranks) and np.array_equal(pu["indptr"], h_csr[0]) and np.array_equal(pu["items"], h_csr[1])
    for k in (5, 10, 20):
        assert np.array_equal(pu["ndcg"][k], m["ndcg"][k]) and np.array_equal(pu["recall"][k], m["recall"][k])
        assert np.array_equal(pu["hit"][k], m["hit"][k])
        assert result[f"n{k}"] == m["sums"]["ndcg"][k] / len(users) and result[f"r{k}"] == m["sums"]["recall"][k] / len(users)
        assert result[f"hr{k}"] == m["sums"]["hit"][k] / len(users)
    assert np.array_equal(pu["rr"], m["rr"]) and result["mrr"] == m["sums"]["rr"] / len(users)


def test_evaluate_catalogue_refusals():
    import torch
    model, user_num, n_items = cpu_model("ncf")
    held, excl = interactions(user_num, n_items)
    with pytest.raises(ValueError, match="impl='cpu'"):
        evaluate_catalogue(model, None, held, impl="cpu")
    with pytest.raises(ValueError, match="ks="):
        evaluate_catalogue(model, None, held, ks=(20, 10), impl="host")
    with pytest.raises(ValueError, match="the held-out set is empty"):
        evaluate_catalogue(model, None, [], impl="host")
    with pytest.raises(ValueError, match=r"heldout: users in \[\d+, \d+\] outside"):
        evaluate_catalogue(model, None, [(user_num, 0)], impl="host")
    with pytest.raises(ValueError, match=r"heldout: held-out items in \[\d+, \d+\] outside"):
        evaluate_catalogue(model, None, [(0, n_items)], impl="host")
    with pytest.raises(ValueError, match=r"exclude: excluded items in \[-1, -1\] outside"):
        evaluate_catalogue(model, None, held, exclude=[(0, -1)], impl="host")
    with pytest.raises(ValueError, match=f"3 of {len(held)} held-out pairs are also excluded"):
        evaluate_catalogue(model, None, held, exclude=excl + held[:3], impl="host")
    with pytest.raises(ValueError, match="batch_users = 0"):
        evaluate_catalogue(model, None, held, batch_users=0, impl="host")
    with pytest.raises(ValueError, match="evaluate_catalogue: .*item table"):
        evaluate_catalogue(model, None, held, impl="host", table=torch.zeros(n_items, 3))
    gmf, _, _ = cpu_model("gmf")
    with pytest.raises(ValueError, match="evaluate_catalogue: kind 'GMF' reads no item table"):
        evaluate_catalogue(gmf, None, held, impl="host", table=torch.zeros(n_items, 16))
    # a NaN: eligible for two evaluated users' rows (everyone's, minus those who exclude the item), named by their number
    table = model.embed_item_MLP.weight.detach().clone()
    table[4, 1] = float("nan")
    few = [(0, 1), (2, 3), (4, 5)]
    with pytest.raises(ValueError, match="2 of 3 users have a NaN score among their eligible items"):
        evaluate_catalogue(model, None, few, exclude=[(2, 4)], impl="host", table=table)
    evaluate_catalogue(model, None, few, exclude=[(0, 4), (2, 4), (4, 4)], impl="host", table=table)      # excluded for all: no error
    # an uncovered head is refused by the existing check, before anything runs (no GPU is touched)
    from pmgt_amd.ncf import NCF
    odd = NCF(user_num, n_items, 12, 2, model="MLP")
    with pytest.raises(ValueError) as e:
        evaluate_catalogue(odd, None, few, impl="device")
    from pmgt_amd.ncf_model import check_ncf_model_covered
    with pytest.raises(ValueError) as want:
        check_ncf_model_covered(12, 2, "MLP", odd.layer_norm_eps)
    assert str(e.value) == str(want.value)
