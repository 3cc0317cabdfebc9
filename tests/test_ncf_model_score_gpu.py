"""pmgt_ncf_model_score on synthetic models of the stand-alone NCF class: the fused fp32 head with LayerNorm, kind GMF and NeuMF-pre against
the fp64 formula, with the error of the fp32 formula as the measure (tests/ncf_model_score_util.py's header; the models are chosen on the
CPU, tests/test_ncf_model_score_cpu.py asserts that they can judge a kernel).  Condition per case:
    max|kernel - o64| <= 4 max(max|r32 - o64|, 2^-22 max|o64|),    o64 / r32 = ncf_model_scores_host in fp64 / fp32.
The heads are scored once at the largest (n, I) on the host; every smaller case is judged against its block of that reference."""
import ctypes as C

import numpy as np
import pytest
import torch

from pmgt_amd.recommend import NcfModelScorer, NcfScorer
from tests.ncf_model_score_util import C_BOUND, EPS, EPS_HEAD, EPS_OTHER, HEADS, ITEMS, NS, USER_NUM, head_id, model_weights, tensors, users_of, world

pytestmark = pytest.mark.gpu

CANARY = 7777.0


def cut(w, n_items):
    """the model over the first n_items items"""
    return {k: (v[:n_items] if k.startswith("embed_item_") else v) for k, v in w.items()}


def judge(h, eps):
    wd = tensors(h["w"])
    users, o64, r32, head = h["users"], h["o64"], h["r32"], h["head"]
    worst = 0.0
    for n_items in ITEMS:
        scorer = NcfModelScorer(cut(wd, n_items), None, h["kind"], eps)
        assert scorer.n_items == n_items
        for n in NS:
            out = torch.full((n + 1, n_items + 3), CANARY, device="cuda")
            scorer.score(torch.from_numpy(users[:n].copy()).cuda(), out=out)
            got = out.cpu().numpy()
            assert (got[:, n_items:] == CANARY).all() and (got[n] == CANARY).all(), "wrote outside [n, I]"
            ref, r = o64[:n, :n_items], r32[:n, :n_items]
            e_k, e_r = np.abs(got[:n, :n_items] - ref).max(), np.abs(r - ref).max()
            floor = max(e_r, 2.0 ** -22 * np.abs(ref).max())
            worst = max(worst, e_k / floor)
            print(f"head {head_id(head)} eps {eps:g} n {n} I {n_items}: kernel error {e_k:.3e}, fp32 formula error {e_r:.3e}, ratio {e_k / floor:.2f}")
            assert e_k <= C_BOUND * floor, (head, n, n_items, e_k, e_r)
    print(f"head {head_id(head)} eps {eps:g}: largest ratio kernel error / yardstick {worst:.2f}")


@pytest.mark.parametrize("head", HEADS, ids=head_id)
def test_kernel_within_four_times_the_fp32_formulas_error(head):
    judge(world(head), EPS)


def test_layer_norm_eps_takes_part():
    judge(world(EPS_HEAD, EPS_OTHER), EPS_OTHER)


PMGT_KEYS = {"embed_user_MLP.weight": "mlp_user_embeddings.weight", "embed_user_GMF.weight": "gmf_user_embeddings.weight",
             "embed_item_GMF.weight": "gmf_item_embeddings.weight", "predict_layer.weight": "predict_layer.weight",
             "predict_layer.bias": "predict_layer.bias"}


@pytest.mark.parametrize("head", [(16, 3, "MLP", False), (8, 2, "NeuMF-end", False), (8, 2, "NeuMF-pre", False), (8, 1, "MLP", False)], ids=head_id)
def test_without_layer_norm_the_bits_are_pmgt_ncf_scores(head):
    wd = tensors(model_weights(head, 31, USER_NUM, 65))
    users = torch.from_numpy(users_of()[:9]).cuda()
    got = NcfModelScorer(wd, None, head[2], EPS).score(users)
    as_head = {PMGT_KEYS[k]: v for k, v in wd.items() if k in PMGT_KEYS}
    for i in range(head[1]):
        as_head[f"mlp_layers.{i}.linear.weight"], as_head[f"mlp_layers.{i}.linear.bias"] = wd[f"MLP_layers.{3 * i}.weight"], wd[f"MLP_layers.{3 * i}.bias"]
    want = NcfScorer(as_head, wd["embed_item_MLP.weight"]).score(users)
    assert torch.equal(got, want) and torch.isfinite(got).all() and got.abs().max() > 1e-2


def test_neumf_pre_has_the_bits_of_a_neumf_end_holding_its_tensors():
    wd = tensors(world((8, 2, "NeuMF-pre", True))["w"])
    users = torch.from_numpy(users_of()).cuda()
    pre = NcfModelScorer(wd, None, "NeuMF-pre", EPS).score(users)
    assert torch.equal(pre, NcfModelScorer(wd, None, "NeuMF-end", EPS).score(users))
    assert torch.equal(pre, NcfModelScorer(wd, None, None, EPS).score(users))      # read from the tensors: NeuMF-end


@pytest.mark.parametrize("head", [(8, 1, "MLP", True), (64, 2, "NeuMF-end", True), (32, 4, "MLP", True), (64, 1, "GMF", False)], ids=head_id)
def test_repeatable_and_nan_reaches_exactly_its_item(head):
    h = world(head)
    w = cut(h["w"], 65)
    ud = torch.from_numpy(h["users"][:5].copy()).cuda()
    a = NcfModelScorer(tensors(w), None, h["kind"], EPS).score(ud)
    b = NcfModelScorer(tensors(w), None, h["kind"], EPS).score(ud)
    assert torch.equal(a, b) and torch.equal(a[0], a[3])      # the same bytes again; the same user twice
    bad = {k: np.array(v) for k, v in w.items()}
    bad["embed_item_GMF.weight" if head[2] == "GMF" else "embed_item_MLP.weight"][9, 2] = np.nan
    got = NcfModelScorer(tensors(bad), None, h["kind"], EPS).score(ud).cpu().numpy()
    assert np.isnan(got[:, 9]).all() and not np.isnan(np.delete(got, 9, axis=1)).any()
    if head[2] != "GMF":                                     # a table handed over: the same function of its rows
        table = torch.from_numpy(np.array(w["embed_item_MLP.weight"])).cuda()
        moved = NcfModelScorer(tensors(bad), table, h["kind"], EPS).score(ud)
        assert torch.equal(moved, a)
    else:
        with pytest.raises(ValueError, match="reads no item table"):
            NcfModelScorer(tensors(w), torch.zeros(65, 64, device="cuda"), "GMF", EPS)


def test_gmf_user_outside_the_table_scores_nan():
    from pmgt_amd import _lib
    h = world((8, 2, "GMF", False))
    scorer = NcfModelScorer(tensors(cut(h["w"], 33)), None, "GMF", EPS)
    users = torch.tensor([3, USER_NUM, -1, 4], device="cuda")      # (the host surface refuses such ids; the entry never reads outside)
    got = scorer.score(users).cpu().numpy()
    assert np.isnan(got[1:3]).all() and np.isfinite(got[[0, 3]]).all()
    assert _lib.NCF_MODEL_KINDS.index("GMF") == 2


def test_uncovered_models_are_refused_before_any_launch():
    from pmgt_amd import _lib
    lib = _lib.hip()
    for head, what in (((64, 4, "MLP", True), "above 256"), ((4, 2, "GMF", False), "factor_num")):
        with pytest.raises(ValueError, match=what):
            NcfModelScorer(tensors(model_weights(head, 1, 3, 4)), None, head[2], EPS)
    with pytest.raises(ValueError, match="layer_norm_eps"):
        NcfModelScorer(tensors(model_weights((8, 2, "MLP", True), 1, 3, 4)), None, "MLP", -1.0)
    out = torch.full((2, 8), CANARY, device="cuda")
    buf = torch.zeros(1 << 16, device="cuda")                 # (the widest tensor a valid call below reads: W_1 [128][256])
    users = torch.zeros(2, dtype=torch.int64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = buf.data_ptr()

    def call(factor=8, num_layers=2, kind=0, ln=1, eps=1e-12, n=2, n_items=8, stride=8, pu=p, w1=p, gamma=p, gmf=p):
        h = _lib.NcfModelHeadC()
        h.factor_num, h.num_layers, h.kind, h.use_layer_norm, h.layer_norm_eps, h.user_num = factor, num_layers, kind, ln, eps, 2
        for i in range(min(max(num_layers, 0), 4)):
            h.weight[i], h.bias[i], h.gamma[i], h.beta[i] = w1, p, gamma, p
        h.predict_weight, h.predict_bias, h.gmf_user, h.gmf_item = p, p, gmf, gmf
        return lib.pmgt_ncf_model_score(C.byref(h), pu, p, users.data_ptr(), n, n_items, out.data_ptr(), stride, st)

    bad = [dict(kind=4), dict(kind=-1), dict(factor=64, num_layers=4), dict(factor=64, num_layers=4, kind=1, ln=0), dict(factor=12),
           dict(factor=12, kind=2), dict(num_layers=0), dict(num_layers=5), dict(eps=float("nan")), dict(eps=-1e-6), dict(eps=float("inf")),
           dict(eps=float("nan"), kind=2), dict(gamma=0), dict(gamma=0, num_layers=1), dict(n=0), dict(n=2 ** 20 + 1), dict(n_items=0),
           dict(stride=7), dict(pu=0), dict(pu=p + 2), dict(w1=0), dict(kind=1, gmf=0), dict(kind=2, gmf=0), dict(kind=3, gmf=0),
           dict(stride=7, kind=2), dict(n=0, kind=2), dict(w1=0, ln=0)]
    assert [call(**b) for b in bad] == [-2] * len(bad)
    torch.cuda.synchronize()
    assert (out == CANARY).all()
    # a valid all-zero call of every kind and path: every logit is 0 (gamma = beta = 0, or no LayerNorm)
    for ok in (dict(), dict(kind=1), dict(kind=2), dict(kind=2, num_layers=7, pu=0, w1=0, gamma=0), dict(kind=3), dict(num_layers=1), dict(ln=0),
               dict(kind=3, ln=0, gamma=0), dict(factor=64, num_layers=3), dict(factor=64, num_layers=2, kind=1)):
        out.fill_(CANARY)
        assert call(**ok) == 0, ok
        torch.cuda.synchronize()
        assert (out == 0).all(), ok
