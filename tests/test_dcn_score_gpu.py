"""pmgt_dcn_score and pmgt_dcn_score_rows on synthetic Deep & Cross Networks: the fused fp32 model (the deep tower on the NCF scoring tile,
the collapsed cross net in its epilogue) against the fp64 formula, with the error of the fp32 formula as the measure
(tests/dcn_score_util.py's header; the models are chosen on the CPU, tests/test_dcn_score_cpu.py asserts that they can judge a kernel).
Condition per case:
    max|kernel - o64| <= 4 max(max|r32 - o64|, 2^-22 max|o64|),    o64 / r32 = dcn_scores_host in fp64 / fp32.
The heads are scored once at the largest (n, I) on the host; every smaller case is judged against its block of that reference."""
import ctypes as C

import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.dcn_head import ITEM_KEY, USER_KEY, dcn_layout, dcn_row_scalars_host
from pmgt_amd.recommend import DcnScorer
from tests.dcn_score_util import C_BOUND, EPS, EPS_HEAD, EPS_OTHER, HEADS, ITEMS, NS, USER_NUM, head_id, tensors, world
from tests.dcn_util import torch_model

pytestmark = pytest.mark.gpu

CANARY = 7777.0
RS = _lib.DCN_SCORE_ROW_STRIDE


def cut(w, n_items):
    """the model over the first n_items items"""
    return {k: (v[:n_items] if k == ITEM_KEY else v) for k, v in w.items()}


def judge(h, eps):
    wd = tensors(h["w"])
    users, o64, r32, head = h["users"], h["o64"], h["r32"], h["head"]
    worst = 0.0
    for n_items in ITEMS:
        scorer = DcnScorer(cut(wd, n_items), None, eps)
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


@pytest.mark.parametrize("head", HEADS, ids=head_id)
def test_row_scalars_against_numpy(head):
    """pmgt_dcn_score_rows on the rows of both halves: mu, q and every d_c within the measure of numpy's fp32 against numpy's fp64, per column;
    the columns behind the C + 3 values are zeros, and a canary row behind the output stays"""
    h = world(head)
    w, C_layers, ln = h["w"], head[2], head[3]
    scorer = DcnScorer(tensors(cut(w, 65)), None, EPS)
    for half, rows in ((0, w[USER_KEY]), (1, w[ITEM_KEY][:65])):
        got = scorer.rows(torch.from_numpy(np.array(rows)).cuda(), half).cpu().numpy()
        assert got.shape == (len(rows), RS) and not got[:, C_layers + 3:].any()
        o64, r32 = dcn_row_scalars_host(w, rows, half, np.float64), dcn_row_scalars_host(w, rows, half, np.float32).astype(np.float64)
        if not ln:
            assert not got[:, :2].any()
        for col in range(C_layers + 3):
            e_k, e_r = np.abs(got[:, col] - o64[:, col]).max(), np.abs(r32[:, col] - o64[:, col]).max()
            floor = max(e_r, 2.0 ** -22 * np.abs(o64[:, col]).max())
            print(f"head {head_id(head)} half {half} rows {len(rows)} column {col}: ratio {e_k / floor if floor else 0.0:.2f}")
            assert e_k <= C_BOUND * floor, (head, half, col, e_k, e_r)
    items = torch.from_numpy(np.array(w[ITEM_KEY][:65])).cuda()
    assert torch.equal(scorer.item_rows, scorer.rows(items, 1)) and torch.equal(scorer.item_rows[:1], scorer.rows(items[:1], 1))      # one row alone


@pytest.mark.parametrize("head", [(16, 1, 4, True), (64, 1, 6, False), (16, 2, 2, False), (64, 2, 6, True), (16, 4, 2, True)], ids=head_id)
def test_repeatable_and_nan_reaches_exactly_its_item_or_its_user(head):
    h = world(head)
    w = cut(h["w"], 65)
    ud = torch.from_numpy(h["users"][:5].copy()).cuda()
    a = DcnScorer(tensors(w), None, EPS).score(ud)
    b = DcnScorer(tensors(w), None, EPS).score(ud)
    assert torch.equal(a, b) and torch.equal(a[0], a[3]) and torch.isfinite(a).all()      # the same bytes again; the same user twice
    bad = {k: np.array(v) for k, v in w.items()}
    bad[ITEM_KEY][9, 2] = np.nan
    got = DcnScorer(tensors(bad), None, EPS).score(ud).cpu().numpy()
    assert np.isnan(got[:, 9]).all() and np.array_equal(np.delete(got, 9, axis=1), np.delete(a.cpu().numpy(), 9, axis=1))
    # a table handed over: the same function of its rows
    moved = DcnScorer(tensors(bad), torch.from_numpy(np.array(w[ITEM_KEY])).cuda(), EPS).score(ud)
    assert torch.equal(moved, a)
    bad = {k: np.array(v) for k, v in w.items()}
    bad[USER_KEY][h["users"][1], 5] = np.nan                 # (users[1] appears once among the five)
    assert (h["users"][:5] == h["users"][1]).sum() == 1
    got = DcnScorer(tensors(bad), None, EPS).score(ud).cpu().numpy()
    assert np.isnan(got[1]).all() and np.array_equal(np.delete(got, 1, axis=0), np.delete(a.cpu().numpy(), 1, axis=0))


def test_user_outside_the_table_scores_nan():
    h = world((8, 2, 3, True))
    scorer = DcnScorer(tensors(cut(h["w"], 33)), None, EPS)
    # (the host surface refuses such ids; index_select would fault on them, so the entry is called on rows gathered for valid ids)
    valid = torch.tensor([3, 5, 6, 4], device="cuda")
    users = torch.tensor([3, USER_NUM, -1, 4], device="cuda")
    rows = scorer._user_table.index_select(0, valid)
    out = torch.full((4, 33), CANARY, device="cuda")
    pu, user_rows = rows @ scorer._w0u_t, scorer.rows(rows, 0)      # (held: a temporary's memory would be handed to the next allocation)
    rc = scorer.lib.pmgt_dcn_score(C.byref(scorer._head), pu.data_ptr(), scorer.pi.data_ptr(), user_rows.data_ptr(),
                                   scorer.item_rows.data_ptr(), scorer._consts.data_ptr(), users.data_ptr(), 4, 33, out.data_ptr(), 33,
                                   _lib.stream())
    assert rc == 0
    got = out.cpu().numpy()
    assert np.isnan(got[1:3]).all() and np.array_equal(got[[0, 3]], scorer.score(valid).cpu().numpy()[[0, 3]])


@pytest.mark.parametrize("head", [(16, 1, 4, True), (32, 3, 3, True)], ids=head_id)
def test_a_trainers_flat_buffer_is_read_in_place_with_the_bits_of_the_state_dict(head):
    from pmgt_amd.dcn_train import DcnTrainer, _flat_of
    h = world(head)
    w = cut(h["w"], 65)
    model = torch_model({k: np.array(v) for k, v in w.items()}, head, device="cuda")
    trainer = DcnTrainer(model)
    dims, flat = _flat_of(model)
    assert flat.data_ptr() == trainer.params.data_ptr()
    in_place = DcnScorer((dims, flat), None, EPS)
    assert in_place.flat.data_ptr() == trainer.params.data_ptr()
    ud = torch.from_numpy(h["users"][:9].copy()).cuda()
    gathered = DcnScorer({k: v for k, v in model.state_dict().items()}, None, EPS)
    assert gathered.flat.data_ptr() != trainer.params.data_ptr()
    assert torch.equal(in_place.score(ud), gathered.score(ud)) and torch.equal(in_place.score(ud), DcnScorer(tensors(w), None, EPS).score(ud))


def test_refusals_write_nothing_and_zero_models_score_zero():
    lib = _lib.hip()
    out = torch.full((2, 8), CANARY, device="cuda")
    count = max(dcn_layout(f, l, c, True, 2, 8)[1] for f, l, c in ((64, 2, 6), (16, 4, 1), (64, 1, 6)))      # the largest flat buffer a call below reads
    buf = torch.zeros(count + 8, device="cuda")
    users = torch.zeros(2, dtype=torch.int64, device="cuda")
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = buf.data_ptr()

    def call(factor=8, deep=2, cross=2, ln=1, eps=1e-12, n=2, n_items=8, stride=8, params=p, pu=p, pi=p, ur=p, ir=p, consts=p, us=None, scores=None,
             user_num=2, item_num=8):
        h = _lib.DcnHeadC(factor, deep, cross, ln, eps, 0, user_num, item_num, params, None)
        return lib.pmgt_dcn_score(C.byref(h), pu, pi, ur, ir, consts, users.data_ptr() if us is None else us, n, n_items,
                                  out.data_ptr() if scores is None else scores, stride, st)

    def call_rows(factor=8, deep=2, cross=2, ln=1, eps=1e-12, rows=2, half=0, params=p, table=p, dst=None):
        h = _lib.DcnHeadC(factor, deep, cross, ln, eps, 0, 2, 8, params, None)
        return lib.pmgt_dcn_score_rows(C.byref(h), table, rows, half, out.data_ptr() if dst is None else dst, st)

    bad = [dict(factor=12), dict(factor=4), dict(deep=0), dict(deep=5), dict(factor=64, deep=3), dict(cross=0), dict(cross=7), dict(ln=2),
           dict(eps=float("nan")), dict(eps=-1e-6), dict(eps=float("inf")), dict(eps=float("nan"), ln=0), dict(n=0), dict(n=2 ** 20 + 1),
           dict(n_items=0), dict(stride=7), dict(params=0), dict(params=p + 4), dict(pu=0), dict(pu=p + 4), dict(pi=0), dict(pi=p + 8),
           dict(ur=0), dict(ur=p + 4), dict(ir=0), dict(ir=p + 4), dict(consts=0), dict(consts=p + 2), dict(us=0), dict(us=p + 4),
           dict(scores=0), dict(scores=out.data_ptr() + 2), dict(user_num=0), dict(item_num=0), dict(deep=1, n=0), dict(deep=1, stride=7, ln=0)]
    assert [call(**b) for b in bad] == [-2] * len(bad)
    bad_rows = [dict(factor=12), dict(deep=5), dict(cross=7), dict(eps=float("nan")), dict(rows=0), dict(half=2), dict(half=-1), dict(params=0),
                dict(table=0), dict(table=p + 4), dict(dst=0), dict(dst=out.data_ptr() + 4)]
    assert [call_rows(**b) for b in bad_rows] == [-2] * len(bad_rows)
    torch.cuda.synchronize()
    assert (out == CANARY).all()
    # a valid all-zero call on every path (VALU / MFMA x LayerNorm / none, every tile): every logit and every row scalar is 0
    for ok in (dict(), dict(ln=0, consts=0), dict(deep=1), dict(deep=1, ln=0, consts=0), dict(factor=64, deep=2, cross=6),
               dict(factor=64, deep=2, cross=6, ln=0), dict(factor=32, deep=2), dict(factor=32, deep=2, ln=0), dict(factor=16, deep=4, cross=1),
               dict(factor=64, deep=1, cross=6)):
        out.fill_(CANARY)
        assert call(**ok) == 0, ok
        torch.cuda.synchronize()
        assert (out == 0).all(), ok
    rows_out = torch.full((3, RS), CANARY, device="cuda")
    for ok in (dict(), dict(ln=0), dict(factor=64, deep=2, cross=6, half=1)):
        rows_out.fill_(CANARY)
        assert call_rows(dst=rows_out.data_ptr(), **ok) == 0, ok
        torch.cuda.synchronize()
        assert (rows_out[:2] == 0).all() and (rows_out[2] == CANARY).all(), ok
