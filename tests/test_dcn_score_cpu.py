"""The host side of scoring and recommending with the Deep & Cross Network; no GPU.  dcn_scores_host (the yardstick of pmgt_dcn_score)
against dcn_head_host and against the torch class; the collapsed form of the cross net (pmgt_amd/dcn_head.py's header) as a second fp32
realisation, which makes the measure of tests/test_dcn_score_gpu.py sound (tests/dcn_score_util.py's header); recommend(impl="host") on a
CPU model; the surface."""
import os

import numpy as np
import pytest
import torch

from pmgt_amd.dcn_head import dcn_head_host, dcn_row_scalars_host, dcn_score_constants, dcn_scores_host
from pmgt_amd.recommend import DcnScorer, exclusion_csr, recommend, topk_host
from tests.dcn_score_util import (C_BOUND, EPS, EPS_HEAD, EPS_OTHER, FIRST_SEED, HEADS, SEEDS, USER_NUM, case_ratios, head_id, model_weights,
                                  second_realisation, second_worst, world)
from tests.dcn_util import torch_model

HEAD_PARAMS = pytest.mark.parametrize("head", HEADS, ids=head_id)
ITEM = "item_embeddings.weight"


@HEAD_PARAMS
def test_the_yardstick_is_dcn_head_hosts_logits(head):
    """the same pair rows through the same function: the same bits, in both precisions; chunks of whole users change nothing"""
    h = world(head)
    users, n_items = h["users"][:9], 33
    w = {k: (v[:n_items] if k == ITEM else v) for k, v in h["w"].items()}
    pu, pi = np.repeat(users, n_items), np.tile(np.arange(n_items), len(users))
    for dtype in (np.float64, np.float32):
        s = dcn_scores_host(w, users, None, dtype, EPS)
        z = dcn_head_host(w, pu, pi, dtype, EPS)
        assert s.dtype == dtype and s.shape == (len(users), n_items) and np.array_equal(s.reshape(-1), z)
        for r in (0, 5):                                     # a chunk of one user is that user's pair rows
            assert np.array_equal(dcn_scores_host(w, users, None, dtype, EPS, pair_chunk=1)[r], dcn_head_host(w, pu[:n_items] * 0 + users[r],
                                                                                                                pi[:n_items], dtype, EPS))
    # a table handed over stands in for item_embeddings.weight
    table = np.random.default_rng(1).standard_normal(w[ITEM].shape).astype(np.float32)
    moved = dcn_scores_host(dict(w, **{ITEM: table}), users, None, np.float64, EPS)
    assert np.array_equal(dcn_scores_host(w, users, table, np.float64, EPS), moved) and not np.array_equal(moved, s)
    assert np.array_equal(dcn_scores_host(w, users, torch.from_numpy(table), np.float64, EPS), moved)
    with pytest.raises(ValueError, match="item table"):
        dcn_scores_host(w, users, table[:, :-1])
    with pytest.raises(ValueError, match="users"):
        dcn_scores_host(w, np.array([USER_NUM]))


@pytest.mark.parametrize("head", [(16, 1, 4, True), (16, 2, 2, False), (64, 2, 6, True)], ids=head_id)
def test_the_yardstick_against_the_torch_class_in_fp64(head):
    h = world(head)
    users, n_items = h["users"], len(h["o64"][0])
    model = torch_model({k: v.copy() for k, v in h["w"].items()}, head, torch.float64)
    with torch.no_grad():
        z = model((torch.from_numpy(np.repeat(users, n_items)), torch.from_numpy(np.tile(np.arange(n_items), len(users))))).numpy()
    assert np.abs(z.reshape(len(users), n_items) - h["o64"]).max() <= 1e-12 * np.abs(h["o64"]).max()
    assert 1e-2 < np.abs(h["o64"]).max() < 50                 # logits O(1)


@HEAD_PARAMS
def test_the_collapsed_cross_net_is_the_cross_net_in_fp64(head):
    """the form the kernel computes, in fp64: the constants and the row scalars reproduce x^(C) . wo[:D] of the formulae on pair rows"""
    from pmgt_amd.dcn_head import _forward, head_weights
    h = world(head)
    factor, L, C, ln = head
    w = head_weights(h["w"], np.float64)
    users, items = h["users"][:7], np.arange(11)
    pu, pi = np.repeat(users, len(items)), np.tile(items, len(users))
    xs = _forward(w, pu, pi, EPS)[1]
    D = xs[-1].shape[1]
    want = (xs[-1] @ w["output_layer.weight"].reshape(-1)[:D]).reshape(len(users), len(items))
    g, K, B = dcn_score_constants(w)
    su = dcn_row_scalars_host(w, w["user_embeddings.weight"][users], 0)
    si = dcn_row_scalars_host(w, w[ITEM][items], 1)
    assert g.shape == (2, C + 1, D // 2) and su.shape == (len(users), C + 3)
    d = su[:, None, 2:] + si[None, :, 2:]
    if ln:
        m0 = (su[:, None, 0] + si[None, :, 0]) / 2
        v0 = (su[:, None, 1] + si[None, :, 1] + (D // 2) * ((su[:, None, 0] - m0) ** 2 + (si[None, :, 0] - m0) ** 2)) / D
        s = d[:, :, 0]
        for c in range(C):
            k = s + 1
            s = k / np.sqrt(k * k * v0 + EPS) * (d[:, :, c + 1] - m0 * K[c]) + B[c]
        got = s
    else:
        assert not su[:, :2].any() and not K.any() and not B.any()
        m = np.ones_like(want)
        for c in range(C):
            m = m * d[:, :, c] + 1
        got = m * d[:, :, C]
    assert np.abs(got - want).max() <= 1e-11 * max(1.0, np.abs(want).max())


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


@pytest.mark.parametrize("head", [(8, 1, 1, False), (8, 2, 3, True)], ids=head_id)
def test_recommend_on_a_cpu_model_is_topk_host_of_the_yardstick(head):
    n_users, n_items, k = 5, 7, 4
    w = model_weights(head, 3, n_users, n_items)
    model = torch_model(w, head).train()
    users = np.array([0, 1, 4, 1, 3])
    pairs = [(1, j) for j in (0, 1, 2, 3, 5)] + [(3, 6), (4, 0), (4, 2)]      # user 1 keeps two items: fewer than k
    got_items, got_scores = recommend(model, None, users, k=k, exclude=pairs, impl="host")
    assert model.training                                     # the caller's mode is restored
    o64, r32 = (dcn_scores_host(w, users, None, dt, EPS) for dt in (np.float64, np.float32))
    items, scores, flags = topk_host(r32, k, *exclusion_csr(pairs, n_users, n_items), users)
    assert got_items.dtype == np.int64 and got_scores.dtype == np.float32 and np.array_equal(got_items, items)
    assert (got_items[1] >= 0).sum() == 2 and (got_items[3] == got_items[1]).all() and np.isneginf(got_scores[1, 2:]).all()
    live = items >= 0
    # torch's model and numpy's sum a logit in their own orders: the scores agree within the measure of the GPU tests
    tol = C_BOUND * max(np.abs(r32 - o64).max(), 2.0 ** -22 * np.abs(o64).max())
    assert np.abs(got_scores[live].astype(np.float64) - scores[live]).max() <= tol
    model.eval()
    recommend(model, None, users, k=k, impl="host")
    assert not model.training
    # a model with dropout is scored without masks: the same items from a model that differs in its dropout only
    from pmgt_amd.dcn import DCN
    dropped = DCN(n_users, n_items, *head[:3], emb_dropout=0.2, dropout=0.3, use_layer_norm=head[3], layer_norm_eps=EPS)
    dropped.load_state_dict(model.state_dict())
    again = recommend(dropped.train(), None, users, k=k, exclude=pairs, impl="host")
    assert np.array_equal(again[0], got_items) and np.array_equal(again[1], got_scores) and dropped.training
    # refusals of the host surface
    with pytest.raises(ValueError, match="users"):
        recommend(model, None, np.array([n_users]), k=2, impl="host")
    with pytest.raises(ValueError, match="k = "):
        recommend(model, None, users, k=0, impl="host")
    E = head[0] << head[1]
    table = torch.randn(n_items + 1, E)[1:]                   # a view of another buffer
    moved = recommend(model, None, users, k=k, impl="host", table=table)
    want = topk_host(dcn_scores_host(w, users, table, np.float32, EPS), k)
    assert np.array_equal(moved[0], want[0]) and not np.array_equal(moved[0], recommend(model, None, users, k=k, impl="host")[0])
    with pytest.raises(ValueError, match="item table"):
        recommend(model, None, users, k=2, impl="host", table=torch.zeros(n_items, E // 2))


def test_an_uncovered_shape_is_refused_for_the_device_before_a_gpu_is_touched(monkeypatch):
    from pmgt_amd import _lib
    from pmgt_amd.dcn import DCN

    def no_gpu(*a, **k):
        raise AssertionError("the device library was loaded")
    monkeypatch.setattr(_lib, "hip", no_gpu)
    users = np.array([0, 1])
    for kwargs, what in ((dict(factor_num=12, deep_net_num_layers=1), "factor_num"), (dict(factor_num=64, deep_net_num_layers=3), "above 256"),
                         (dict(factor_num=8, deep_net_num_layers=1, cross_net_num_layers=7), "cross_net_num_layers")):
        model = DCN(3, 4, **kwargs)
        with pytest.raises(ValueError, match=what):
            recommend(model, None, users, k=2, impl="device")
        items, scores = recommend(model, None, users, k=2, impl="host")      # the host path has no such limit
        assert items.shape == (2, 2) and np.isfinite(scores).all()
    with pytest.raises(ValueError, match="factor_num"):
        DcnScorer({k: v for k, v in DCN(3, 4, factor_num=12, deep_net_num_layers=1).state_dict().items()})


def test_surface():
    import ctypes as C

    import pmgt_amd
    from pmgt_amd import _build, _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "pmgt_capi.h")).read()
    assert {"pmgt_dcn_score", "pmgt_dcn_score_rows"} <= set(_lib.HIP_SYMBOLS) and "pmgt_dcn_score(" in hdr and "pmgt_dcn_score_rows(" in hdr
    assert f"enum {{ PMGT_DCN_SCORE_ROW_STRIDE = {_lib.DCN_SCORE_ROW_STRIDE} }};" in hdr
    assert _lib.DCN_SCORE_ROW_STRIDE % 4 == 0 and _lib.DCN_SCORE_ROW_STRIDE >= _lib.DCN_MAX_CROSS + 3      # mu, q, d_0 .. d_C
    assert any(p.endswith(os.path.join("ops", "dcn_score.hip")) for p in _build.OPS_SOURCES)
    assert pmgt_amd.dcn_scores_host is dcn_scores_host and pmgt_amd.DcnScorer is DcnScorer
    assert C.sizeof(_lib.DcnHeadC) == 6 * 4 + 4 * 8           # pmgt_dcn_head as the entries read it: unchanged
