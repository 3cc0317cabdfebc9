"""pmgt_ncf_score on synthetic heads: the fused fp32 head against the fp64 formula, with the error of the fp32 formula as the measure.

Yardsticks per head: o64 = ncf_head_host(..., np.float64); r32 = the same formula in fp32 numpy on the UNSPLIT layer 0, i.e. what the torch
head computes.  Condition per case:  max|kernel - o64| <= 4 max(max|r32 - o64|, 2^-22 max|o64|).
The kernel adds one rounding by splitting layer 0 and accumulates in MFMA block order; both differ from r32 by reordering only, so the error
classes are the same.  A bf16 operand (about 2^-8 relative), a dropped bias or a missing ReLU misses by orders of magnitude.

The heads are scored once at the largest (n, I) on the host; a pair's logit does not depend on the other pairs, so every smaller case is
judged against its block of that reference."""
import ctypes as C

import numpy as np
import pytest
import torch

from pmgt_amd.recommend import NcfScorer, ncf_head_host
from tests.test_recommend_cpu import random_head

pytestmark = pytest.mark.gpu

HEADS = [(8, 1, "MLP"), (8, 4, "MLP"), (16, 3, "MLP"), (32, 3, "NeuMF-end"), (64, 3, "NeuMF-end"), (64, 2, "MLP")]
NS, ITEMS = (1, 5, 67), (1, 63, 65, 300, 1000)
USER_NUM = 80
CANARY = 7777.0


@pytest.fixture(scope="module", params=HEADS, ids=lambda h: f"f{h[0]}-L{h[1]}-{h[2]}")
def head(request):
    factor, num_layers, kind = request.param
    w, table = random_head(factor, num_layers, kind, USER_NUM, ITEMS[-1], seed=1000 + 10 * factor + num_layers)
    users = np.random.default_rng(7).integers(0, USER_NUM, size=NS[-1])
    users[3] = users[0]                                      # a user twice
    return dict(shape=request.param, w=w, table=table, users=users, o64=ncf_head_host(w, users, table, np.float64),
                r32=ncf_head_host(w, users, table, np.float32).astype(np.float64))


def test_kernel_within_four_times_the_fp32_formulas_error(head):
    w, table, users, o64, r32 = head["w"], head["table"], head["users"], head["o64"], head["r32"]
    wd = {k: torch.from_numpy(v).cuda() for k, v in w.items()}
    worst = 0.0
    for n_items in ITEMS:
        scorer = NcfScorer(wd, torch.from_numpy(table[:n_items]).cuda())
        for n in NS:
            out = torch.full((n + 1, n_items + 3), CANARY, device="cuda")
            scorer.score(torch.from_numpy(users[:n]).cuda(), out=out)
            got = out.cpu().numpy()
            assert (got[:, n_items:] == CANARY).all() and (got[n] == CANARY).all(), "wrote outside [n, I]"
            ref, r = o64[:n, :n_items], r32[:n, :n_items]
            e_k, e_r = np.abs(got[:n, :n_items] - ref).max(), np.abs(r - ref).max()
            bound = 4 * max(e_r, 2.0 ** -22 * np.abs(ref).max())
            ratio = e_k / max(e_r, 2.0 ** -22 * np.abs(ref).max())
            worst = max(worst, ratio)
            print(f"head {head['shape']} n {n} I {n_items}: kernel error {e_k:.3e}, fp32 formula error {e_r:.3e}, ratio {ratio:.2f}")
            assert e_k <= bound, (head["shape"], n, n_items, e_k, e_r)
    print(f"head {head['shape']}: largest ratio kernel error / yardstick {worst:.2f}")
    assert 1e-2 < np.abs(o64).max() < 50                     # logits O(1)


def test_repeatable_and_nan_reaches_the_scores(head):
    w, table, users = head["w"], head["table"][:65].copy(), head["users"][:5]
    wd = {k: torch.from_numpy(v).cuda() for k, v in w.items()}
    ud = torch.from_numpy(users).cuda()
    a = NcfScorer(wd, torch.from_numpy(table).cuda()).score(ud)
    b = NcfScorer(wd, torch.from_numpy(table).cuda()).score(ud)
    assert torch.equal(a, b) and torch.equal(a[0], a[3])      # the same bytes again; the same user twice
    table[9, 2] = np.nan
    got = NcfScorer(wd, torch.from_numpy(table).cuda()).score(ud).cpu().numpy()
    assert np.isnan(got[:, 9]).all() and not np.isnan(np.delete(got, 9, axis=1)).any()


def test_uncovered_heads_are_refused_before_any_launch():
    from pmgt_amd import _lib
    lib = _lib.hip()
    for factor, num_layers, what in ((64, 4, "above 256"), (4, 2, "factor_num"), (8, 5, "num_layers")):
        w, table = random_head(factor, num_layers, "MLP", 3, 4, seed=1)
        with pytest.raises(ValueError, match=what):
            NcfScorer({k: torch.from_numpy(v).cuda() for k, v in w.items()}, torch.from_numpy(table).cuda())
    out = torch.full((2, 8), CANARY, device="cuda")
    buf = torch.zeros(4096, device="cuda")
    users = torch.zeros(2, dtype=torch.int64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(factor=8, num_layers=2, kind=0, n=2, n_items=8, stride=8, pu=buf.data_ptr(), w1=buf.data_ptr(), gmf=0):
        h = _lib.NcfHeadC()
        h.factor_num, h.num_layers, h.kind, h.user_num = factor, num_layers, kind, 2
        for i in range(1, min(max(num_layers, 0), 4)):
            h.weight[i], h.bias[i] = w1, buf.data_ptr()
        h.predict_weight, h.predict_bias, h.gmf_user, h.gmf_item = buf.data_ptr(), buf.data_ptr(), gmf, gmf
        return lib.pmgt_ncf_score(C.byref(h), pu, buf.data_ptr(), users.data_ptr(), n, n_items, out.data_ptr(), stride, st)

    bad = [dict(factor=12), dict(factor=128), dict(num_layers=0), dict(num_layers=5), dict(factor=64, num_layers=4), dict(kind=2), dict(n=0),
           dict(n=2 ** 20 + 1), dict(n_items=0), dict(n_items=2 ** 31 - 1, stride=2 ** 31 - 1), dict(stride=7), dict(pu=0), dict(w1=0),
           dict(kind=1), dict(pu=buf.data_ptr() + 2)]
    assert [call(**b) for b in bad] == [-2] * len(bad)
    torch.cuda.synchronize()
    assert (out == CANARY).all()
    assert call() == 0 and call(kind=1, gmf=buf.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (out == 0).all()                                   # all-zero parameters: every logit is 0
