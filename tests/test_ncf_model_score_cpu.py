"""The host side of scoring and recommending with the stand-alone NCF class; no GPU.  ncf_model_scores_host (the yardstick of
pmgt_ncf_model_score) against ncf_model_grad_host and against the torch class; recommend(impl="host") on a CPU model; the surface; and the
soundness of the measure tests/test_ncf_model_score_gpu.py applies (tests/ncf_model_score_util.py's header)."""
import os

import numpy as np
import pytest
import torch

from pmgt_amd.ncf_model import ncf_model_grad_host, ncf_model_scores_host
from pmgt_amd.recommend import NcfModelScorer, exclusion_csr, recommend, topk_host
from tests.ncf_model_score_util import (C_BOUND, EPS, EPS_HEAD, EPS_OTHER, FIRST_SEED, HEADS, SEEDS, USER_NUM, case_ratios, head_id, model_weights,
                                        second_realisation, second_worst, world)
from tests.ncf_model_util import torch_model

HEAD_PARAMS = pytest.mark.parametrize("head", HEADS, ids=head_id)


@HEAD_PARAMS
def test_the_yardstick_is_ncf_model_grad_hosts_forward(head):
    """the same pair rows through the same functions: the same bits, in both precisions"""
    h = world(head)
    users, n_items = h["users"][:9], 33
    w = {k: (v[:n_items] if k.startswith("embed_item_") else v) for k, v in h["w"].items()}
    pu, pi = np.repeat(users, n_items), np.tile(np.arange(n_items), len(users))
    for dtype in (np.float64, np.float32):
        s = ncf_model_scores_host(w, users, None, dtype, EPS, h["kind"])
        z = ncf_model_grad_host(w, pu, pi, np.zeros(len(pu), np.float32), dtype, layer_norm_eps=EPS, kind=h["kind"])[1]
        assert s.dtype == dtype and s.shape == (len(users), n_items) and np.array_equal(s.reshape(-1), z)
    # a table handed over stands in for embed_item_MLP.weight
    if head[2] == "GMF":
        with pytest.raises(ValueError, match="reads no item table"):
            ncf_model_scores_host(w, users, np.zeros((n_items, 8), np.float32), kind="GMF")
    else:
        table = np.random.default_rng(1).standard_normal(w["embed_item_MLP.weight"].shape).astype(np.float32)
        moved = ncf_model_scores_host(dict(w, **{"embed_item_MLP.weight": table}), users, None, np.float64, EPS, h["kind"])
        assert np.array_equal(ncf_model_scores_host(w, users, table, np.float64, EPS, h["kind"]), moved) and not np.array_equal(moved, s)


@HEAD_PARAMS
def test_the_yardstick_against_the_torch_class_in_fp64(head):
    h = world(head)
    users, n_items = h["users"], len(h["o64"][0])
    model = torch_model({k: v.copy() for k, v in h["w"].items()}, head, torch.float64).eval()
    u = torch.from_numpy(np.repeat(users, n_items))
    i = torch.from_numpy(np.tile(np.arange(n_items), len(users)))
    with torch.no_grad():
        z = model.head(u, i, None if head[2] == "GMF" else model.embed_item_MLP(i)).numpy().reshape(len(users), n_items)
    assert np.abs(z - h["o64"]).max() <= 1e-12 * np.abs(h["o64"]).max()
    assert 1e-2 < np.abs(h["o64"]).max() < 50                 # logits O(1)


@pytest.mark.parametrize("head", [(8, 2, "GMF", False), (8, 2, "NeuMF-end", True)], ids=head_id)
def test_recommend_on_a_cpu_model_is_topk_host_of_the_yardstick(head):
    n_users, n_items, k = 5, 7, 4
    w = model_weights(head, 3, n_users, n_items)
    model = torch_model(w, head, user_num=n_users, item_num=n_items).train()
    users = np.array([0, 1, 4, 1, 3])
    pairs = [(1, j) for j in (0, 1, 2, 3, 5)] + [(3, 6), (4, 0), (4, 2)]      # user 1 keeps two items: fewer than k
    got_items, got_scores = recommend(model, None, users, k=k, exclude=pairs, impl="host")
    assert model.training                                     # the caller's mode is restored
    o64, r32 = (ncf_model_scores_host(w, users, None, dt, EPS, head[2]) for dt in (np.float64, np.float32))
    items, scores, flags = topk_host(r32, k, *exclusion_csr(pairs, n_users, n_items), users)
    assert got_items.dtype == np.int64 and got_scores.dtype == np.float32 and np.array_equal(got_items, items)
    assert (got_items[1] >= 0).sum() == 2 and (got_items[3] == got_items[1]).all() and np.isneginf(got_scores[1, 2:]).all()
    live = items >= 0
    # torch's head and numpy's sum a logit in their own orders: the scores agree within the measure of the GPU tests
    tol = C_BOUND * max(np.abs(r32 - o64).max(), 2.0 ** -22 * np.abs(o64).max())
    assert np.abs(got_scores[live].astype(np.float64) - scores[live]).max() <= tol
    # refusals of the host surface
    with pytest.raises(ValueError, match="users"):
        recommend(model, None, np.array([n_users]), k=2, impl="host")
    if head[2] == "GMF":
        with pytest.raises(ValueError, match="reads no item table"):
            recommend(model, None, users, k=2, impl="host", table=torch.zeros(n_items, 16))
    else:
        table = torch.randn(n_items + 1, 16)[1:]              # a view of another buffer
        moved = recommend(model, None, users, k=k, impl="host", table=table)
        want = topk_host(ncf_model_scores_host(w, users, table, np.float32, EPS, head[2]), k)
        assert np.array_equal(moved[0], want[0])
        with pytest.raises(ValueError, match="item table"):
            recommend(model, None, users, k=2, impl="host", table=torch.zeros(n_items, 8))


def test_surface():
    import pmgt_amd
    from pmgt_amd import _build, _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "pmgt_capi.h")).read()
    assert "pmgt_ncf_model_score" in _lib.HIP_SYMBOLS and "pmgt_ncf_model_score(" in hdr and "pmgt_ncf_model_head" in hdr
    assert any(p.endswith(os.path.join("ops", "ncf_model_score.hip")) for p in _build.OPS_SOURCES)
    assert pmgt_amd.ncf_model_scores_host is ncf_model_scores_host and pmgt_amd.NcfModelScorer is NcfModelScorer
    import ctypes as C
    # the struct of the binding lays out as the header's: 8 ints / floats, one int64, 16 + 4 pointers
    assert C.sizeof(_lib.NcfModelHeadC) == 6 * 4 + 8 + 20 * 8 and _lib.NcfModelHeadC.weight.offset == 32


@HEAD_PARAMS
def test_the_measure_is_sound_on_every_case_of_the_gpu_test(head):
    """A second fp32 realisation, right by construction, keeps within C on every case, and SEEDS holds the FIRST such seed from 29 on: the
    device test then judges the kernel and not the list."""
    h = world(head)
    ratios = case_ratios(second_realisation(h["w"], h["users"], head), h["o64"], h["r32"])
    worst = max(ratios, key=ratios.get)
    print(f"{head_id(head)}: the second realisation's largest ratio {ratios[worst]:.2f} at (n, I) = {worst}")
    assert ratios[worst] <= C_BOUND, (head, worst, ratios[worst])
    for seed in range(FIRST_SEED, SEEDS[head]):
        assert second_worst(head, seed) > C_BOUND, (head, seed, "an earlier seed holds too")
    if head == EPS_HEAD:
        g = world(head, EPS_OTHER)
        again = case_ratios(second_realisation(g["w"], g["users"], head, EPS_OTHER), g["o64"], g["r32"])
        assert max(again.values()) <= C_BOUND
        # and the other eps is another function by far more than the bound: a kernel that drops it misses
        floor = max(np.abs(g["r32"] - g["o64"]).max(), 2.0 ** -22 * np.abs(g["o64"]).max())
        assert np.abs(h["o64"] - g["o64"]).max() > 1e3 * C_BOUND * floor
    assert len(h["users"]) == 67 and h["users"].max() < USER_NUM and h["users"][3] == h["users"][0]
