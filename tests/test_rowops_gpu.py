"""Operator tests of the row kernels of the training step that the per-kernel file (test_ops_gpu.py) does not reach: the embedding mix
(rowops.hip: embed_mix_fwd / _bwd, the embed_tok8 token phase, pos_role_finish), the per-node segment sums (segsum.hip), the loss heads
(loss.hip: gsr, nfr_diff, loss_finish, pair_offsets, nfr_compact, scatter_rows) and the optimizer (optim.hip: clip + AdamW, the weight
mirror).  Each kernel is called through its pmgt_op_* entry (include/pmgt_ops.h), i.e. through the engine's own host function and
dispatch, and compared with a float64 torch restatement of the same operation (oracle/pmgt_oracle.py: embeddings_fwd from the projected
rows on, gsr_loss, nfr_loss, clip_grad_norm, adamw_step; backward passes by autograd in float64).

Judging: element-wise bounds, never cosine.  A float result passes when every element satisfies
    |out - ref| <= ulps * ulp(ref) + floor * max|ref|
with ulp() in the output's storage type: the rounding of the stored value plus the fp32 arithmetic of the kernel (relative to the tensor's
scale).  The reference takes the inputs as the kernel sees them (rounded to the storage type); where a kernel rounds an intermediate that
it stores and re-reads (the pre-LayerNorm sum of the embedding), the reference reads that stored value (straight-through: the value is the
kernel's, the gradient the identity), and the stored intermediate itself is checked against the reference.  Integer work (offsets,
compaction, copies, transposes, segment sums of integer-valued rows) is asserted bit-exact.  Every output buffer starts as NaN (or -7 for
integers), and what lies outside the rows / columns a kernel owns must still hold it afterwards.

Contracts that differ from a literal reading of the reference, tested as such:
  * GSR: a CLS row of norm 0 is normalised by max(|z|, 1e-12) as F.normalize does; its gradient is the one autograd gives through that
    clamp (g / 1e-12: the clamp blocks the norm's own gradient), not zero.
  * loss_finish: a step without masked positions gives a NaN NFR term and a NaN total loss, as the reference's mean over no rows
    (quirk Q2); the GSR term stays finite.
  * pos_role_finish: position rows S .. max_pos - 1 are written as zeros (accumulate: left as they were); rows past max_pos are not
    touched.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = pytest.mark.gpu

DT = {"fp32": (0, torch.float32), "bf16": (1, torch.bfloat16)}
NAN = float("nan")
EPS_LN = 1e-12


def _lib():
    from pmgt_amd import _lib
    return _lib


def H():
    return _lib().hip()


def check(rc):
    _lib().check(rc)


def P(t):
    """device pointer of t: bind the tensor to a name first -- a temporary may be freed (and its block handed to the next allocation on
    the stream) before the kernel that reads it is enqueued"""
    return C.c_void_p(0 if t is None else t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def nans(shape, tdt=torch.float32):
    return torch.full(shape, NAN, device="cuda", dtype=tdt)


def ulp(x, tdt):
    """one unit in the last place of |x| in the storage type tdt (x: float64)"""
    mant = 7 if tdt == torch.bfloat16 else 23
    return torch.exp2(torch.floor(torch.log2(x.abs().clamp_min(1e-30))) - mant)


def assert_close(out, ref, tdt, ulps=None, floor=2e-5, what=""):
    """element-wise |out - ref| <= ulps * ulp(ref) + floor * max|ref|  (NaN fails)"""
    out = out.detach().double()
    ref = ref.detach().double().to(out.device)
    assert out.shape == ref.shape, (what, out.shape, ref.shape)
    if ulps is None:
        ulps = 2.0 if tdt == torch.bfloat16 else 8.0
    scale = ref.abs().max() if ref.numel() else torch.zeros((), dtype=torch.float64, device=out.device)
    bound = ulps * ulp(ref, tdt) + floor * scale
    err = (out - ref).abs()
    bad = ~(err <= bound)
    if bool(bad.any()):
        i = int(torch.nonzero(bad.flatten())[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {ref.numel()} elements out of bound; first at flat index {i}: "
                             f"out {float(out.flatten()[i])!r} ref {float(ref.flatten()[i])!r} bound {float(bound.flatten()[i])!r} "
                             f"(scale {float(scale)!r})")


def all_nan(t):
    return bool(torch.isnan(t.float()).all()) if t.numel() else True


# =========================================================================================== embedding mix
def _embed_args(dt, phase, M, S, d, nf, **bufs):
    L = _lib()
    a = L.EmbedArgsC()
    a.dtype, a.phase, a.M, a.S, a.d, a.nf, a.eps = DT[dt][0], phase, M, S, d, nf, EPS_LN
    for k, v in bufs.items():
        setattr(a, k, v.data_ptr() if torch.is_tensor(v) else v)
    return a


def _embed_params(nf, d, max_pos, g):
    return dict(Wa=torch.randn(nf, nf * d, generator=g) * (2.0 / math.sqrt(nf * d)), ba=torch.randn(nf, generator=g) * 0.7,
                pos=torch.randn(max_pos, d, generator=g) * 0.4, role=torch.randn(2, d, generator=g) * 0.4,
                gamma=1.0 + 0.3 * torch.randn(d, generator=g), beta=0.2 * torch.randn(d, generator=g))


def _mix_ref(Er, Wa, ba, nf, d):
    """a = softmax(Wa tanh(e) + ba), f = sum_k a_k e_k  (oracle embeddings_fwd, from the projected rows on)"""
    a = torch.softmax(torch.tanh(Er) @ Wa.T + ba, -1)
    return a, (a.unsqueeze(-1) * Er.view(-1, nf, d)).sum(1)


def _token_ref(f, prm, S, pre_k, keep):
    """x = f + pos[s] + role[s > 0]; the LayerNorm reads the stored sum pre_k; h0 = dropout(LN(x))"""
    M, d = f.shape
    s = torch.arange(M, device=f.device) % S
    x = f + prm["pos"][s] + prm["role"][(s > 0).long()]
    xs = x + (pre_k - x).detach()
    mean = xs.mean(-1)
    rstd = 1.0 / torch.sqrt(xs.var(-1, unbiased=False) + EPS_LN)
    h = Fn.layer_norm(xs, (d,), prm["gamma"], prm["beta"], EPS_LN) * keep
    return x, xs, torch.stack([mean, rstd], 1), h


def _reduce_parts(part, M, d, nf):
    L = H()
    parts, pe = L.pmgt_op_embed_bwd_parts(M), L.pmgt_op_embed_part_elems(d, nf)
    assert pe == (2 + nf * nf) * d + 4
    assert all_nan(part[parts * pe:]), "partials past the last workgroup"
    s = part[:parts * pe].view(parts, pe).double().sum(0)
    return dict(gamma=s[:d], beta=s[d:2 * d], Wa=s[2 * d:(2 + nf * nf) * d].view(nf, nf * d), ba=s[(2 + nf * nf) * d:(2 + nf * nf) * d + nf],
                pad=s[(2 + nf * nf) * d + nf:])


def _run_embed(dt, phase, nf, d, M, S, n_rows, drop_p=0.0, store_pre=True, seed=0):
    """One forward + backward of the given phase through the pmgt_op_embed_mix entries; returns kernel outputs and fp64 reference."""
    L = H()
    code, tdt = DT[dt]
    g = torch.Generator().manual_seed(seed * 1000 + 17 * d + 5 * nf + M + phase)
    max_pos = S + 7
    prm = _embed_params(nf, d, max_pos, g)
    width = d if phase == 2 else nf * d
    n_src = n_rows if n_rows else M
    E = (torch.randn(n_src, width, generator=g) * 0.8).to(tdt)
    e_rows = torch.randint(0, n_src, (M,), generator=g) if n_rows else None
    if e_rows is not None:
        e_rows[: min(M, 5)] = e_rows[0].item()                    # duplicated rows
    dh0 = torch.randn(M, d, generator=g).to(tdt)
    dF_in = torch.randn(M, d, generator=g) * 0.5                   # phase 1 backward input (segment sums)
    dev = {k: v.cuda() for k, v in prm.items()}
    Ed = E.cuda()
    erd = e_rows.cuda() if e_rows is not None else None
    rng = torch.tensor([4321, 9], dtype=torch.int64, device="cuda") if drop_p > 0 else None
    o = dict(a=nans((M + 1, nf)), pre=nans((M + 1, d), tdt), stats=nans((M + 1, 2)), h0=nans((M + 1, d), tdt))
    fwd = dict(E=Ed, e_rows=erd if erd is not None else 0, a=o["a"], pre=o["pre"] if store_pre else 0, stats=o["stats"], h0=o["h0"],
               drop_p=drop_p, drop_site=3, rng=rng if rng is not None else 0, **{k: dev[k] for k in prm})
    L.pmgt_launch_trace_reset()
    check(L.pmgt_op_embed_mix_fwd(C.byref(_embed_args(dt, phase, M, S, d, nf, **fwd)), stream()))
    tok8_fwd = L.pmgt_launch_trace_count(b"embed_tok8")
    parts, pe = L.pmgt_op_embed_bwd_parts(M), L.pmgt_op_embed_part_elems(d, nf)
    b = dict(dE=nans((M + 1, nf * d), tdt), part=nans(((parts + 1) * pe,)))
    dF32 = phase == 1 and dt == "bf16" and M % 2 == 1
    if phase == 1:
        b["dF"] = (dF_in if dF32 else dF_in.to(tdt)).cuda()
    else:
        b["dF"] = nans((M + 1, d), tdt)
    bwd = dict(fwd, dh0=dh0.cuda(), dE=b["dE"], dF=b["dF"], dF_f32=int(dF32), part=b["part"])
    check(L.pmgt_op_embed_mix_bwd(C.byref(_embed_args(dt, phase, M, S, d, nf, **bwd)), stream()))
    torch.cuda.synchronize()
    tok8_all = L.pmgt_launch_trace_count(b"embed_tok8")

    # ---- fp64 reference on the rounded inputs
    r = {k: v.double().requires_grad_(True) for k, v in prm.items()}
    src = E.double()[e_rows] if e_rows is not None else E.double()
    Er = src.clone().requires_grad_(True)
    ref = {}
    h0k = o["h0"][:M].double().cpu()
    keep = torch.ones(M, d, dtype=torch.float64)
    if drop_p > 0:
        keep = (h0k != 0).double() / (1.0 - drop_p)
    if phase != 2:
        a, f = _mix_ref(Er, r["Wa"], r["ba"], nf, d)
        ref["a"] = a
    else:
        f = Er
    if phase == 1:
        ref["pre"] = f
        f.backward(b["dF"][:M].double().cpu())
    else:
        if store_pre:
            pre_k = o["pre"][:M].double().cpu()
        else:       # what embed_tok8 recomputes: (F + pos) + role in fp32, rounded to bf16
            s = torch.arange(M) % S
            pre_k = ((E[e_rows].float() + prm["pos"][s]) + prm["role"][(s > 0).long()]).to(tdt).double()
        x, xs, stats, h = _token_ref(f, r, S, pre_k, keep)
        xs.retain_grad()
        ref.update(pre=x, stats=stats, h0=h)
        h.backward(dh0.double())
        ref["dF"] = xs.grad
    ref.update(dE=Er.grad, dWa=r["Wa"].grad, dba=r["ba"].grad, dgamma=r["gamma"].grad, dbeta=r["beta"].grad)
    return dict(o=o, b=b, ref=ref, tdt=tdt, tok8=(tok8_fwd, tok8_all), keep=keep, store_pre=store_pre)


def _check_embed(res, phase, nf, d, M):
    o, b, ref, tdt = res["o"], res["b"], res["ref"], res["tdt"]
    f32 = torch.float32
    if phase != 2:
        assert_close(o["a"][:M].cpu(), ref["a"], f32, what="a")
        assert all_nan(o["a"][M:])
    else:
        assert all_nan(o["a"]), "the token phase writes no modality weights"
    if phase == 1:
        assert_close(o["pre"][:M].cpu(), ref["pre"], tdt, what="F (pre)")
        assert all_nan(o["pre"][M:]) and all_nan(o["stats"]) and all_nan(o["h0"]), "the node phase writes F only"
    else:
        if res["store_pre"]:
            assert_close(o["pre"][:M].cpu(), ref["pre"], tdt, what="pre")
        else:
            assert all_nan(o["pre"]), "recompute form: the pre-LayerNorm sum is not stored"
        assert_close(o["stats"][:M].cpu(), ref["stats"], f32, what="stats")
        assert_close(o["h0"][:M].cpu(), ref["h0"], tdt, what="h0")
        for k in ("pre", "stats", "h0"):
            assert all_nan(o[k][M:]), k
    red = _reduce_parts(b["part"], M, d, nf)
    if phase != 1:
        assert_close(b["dF"][:M].cpu(), ref["dF"], tdt, what="dF")
        assert all_nan(b["dF"][M:])
        assert_close(red["gamma"].cpu(), ref["dgamma"], f32, what="dgamma")
        assert_close(red["beta"].cpu(), ref["dbeta"], f32, what="dbeta")
    else:
        assert float(red["gamma"].abs().max()) == 0 and float(red["beta"].abs().max()) == 0, "node phase: no LayerNorm partials"
    if phase != 2:
        assert_close(b["dE"][:M].cpu(), ref["dE"], tdt, what="dE")
        assert all_nan(b["dE"][M:])
        assert_close(red["Wa"].cpu(), ref["dWa"], f32, what="dWa")
        assert_close(red["ba"].cpu(), ref["dba"], f32, what="dba")
    else:
        assert all_nan(b["dE"]), "the token phase writes no dE"
        assert float(red["Wa"].abs().max()) == 0 and float(red["ba"].abs().max()) == 0, "token phase: dWa / dba partials are zero"
    if red["pad"].numel():
        assert float(red["pad"].abs().max()) == 0, "dba padding"


EMBED_CASES = [
    # dt, phase, nf, d, M, S, n_rows (e_rows: token m reads row e_rows[m] of n_rows)
    ("fp32", 0, 1, 32, 77, 9, None),
    ("bf16", 0, 2, 256, 200, 32, None),
    ("fp32", 0, 3, 384, 130, 31, 40),       # NCH = 2 with idle lanes, duplicated rows
    ("bf16", 0, 4, 1024, 67, 64, None),     # NCH = 4
    ("bf16", 0, 1, 512, 95, 9, 30),
    ("fp32", 0, 2, 1024, 129, 64, None),
    ("fp32", 0, 4, 256, 63, 31, None),
    ("bf16", 0, 3, 32, 300, 32, 17),
    ("fp32", 1, 2, 256, 50, 32, None),
    ("bf16", 1, 4, 384, 71, 32, None),      # (odd M: fp32 dF, the segment sums' type)
    ("bf16", 1, 1, 1024, 33, 32, None),
    ("fp32", 1, 3, 32, 129, 32, None),
    ("bf16", 1, 2, 512, 66, 32, None),
    ("bf16", 1, 3, 256, 67, 32, None),
    ("fp32", 2, 2, 384, 93, 31, 20),
    ("fp32", 2, 1, 256, 130, 9, 11),
    ("bf16", 2, 3, 512, 96, 32, 25),
    ("bf16", 2, 2, 32, 201, 9, 7),
    ("bf16", 2, 4, 1024, 128, 64, 50),
]


@pytest.mark.parametrize("dt,phase,nf,d,M,S,n_rows", EMBED_CASES)
def test_embed_mix_matches_fp64(dt, phase, nf, d, M, S, n_rows):
    """Every template instance of embed_mix_fwd / _bwd (fp32 / bf16, phases 0 / 1 / 2, NF = 1..4, NCH = 1 / 2 / 4 with idle lanes at
    d = 384, M off the 4-row and 64-row grids, S in {9, 31, 32, 64} < max_pos): a, pre, stats, h0, dF, dE and the reduced partials."""
    res = _run_embed(dt, phase, nf, d, M, S, n_rows)
    assert res["tok8"] == (0, 0), "only bf16, phase 2, d = 256 with e_rows takes the tok8 kernel"
    _check_embed(res, phase, nf, d, M)


@pytest.mark.parametrize("S,Tq,store_pre", [(32, 7, True), (32, 7, False), (9, 13, False), (31, 5, True), (64, 3, False)])
def test_embed_tok8_token_phase(S, Tq, store_pre):
    """The bench path's token phase (bf16, d = 256, e_rows): the tok8 kernel is dispatched (launch trace), with the stored sum and
    in the recompute form (pre == NULL: the backward rebuilds the sum from F_all, pos and role); odd S leaves half a task idle."""
    M = S * Tq
    res = _run_embed("bf16", 2, 2, 256, M, S, 40, store_pre=store_pre, seed=1)
    assert res["tok8"] == (1, 1 if store_pre else 2), res["tok8"]
    _check_embed(res, 2, 2, 256, M)


@pytest.mark.parametrize("dt,nf,d,store_pre", [("bf16", 2, 256, False), ("fp32", 3, 384, True), ("bf16", 1, 64, True)])
def test_embed_dropout_mask_is_the_one_the_backward_applies(dt, nf, d, store_pre):
    """h0 = dropout(LN(x)): the zero pattern of h0 is the mask the backward applies to dh0 (the reference builds dF from THAT mask), the
    kept values carry 1 / (1 - p), and the keep rate is 1 - p."""
    p = 0.1
    S, Tq = 32, 12
    phase = 2 if dt == "bf16" and d == 256 else 0
    res = _run_embed(dt, phase, nf, d, S * Tq, S, 60, drop_p=p, store_pre=store_pre, seed=3)
    keep = res["keep"] != 0
    assert abs(float(keep.double().mean()) - (1 - p)) < 0.02
    _check_embed(res, phase, nf, d, S * Tq)


def _seg_sum(ids_d, src, n_rows, in_code, out_code, cols=None):
    """sort + segment sums through the pmgt_op entries (the engine's table-mode backward)"""
    L = H()
    M = ids_d.numel()
    cols = cols or src.shape[1]
    mk = lambda n: torch.full((n,), -7, dtype=torch.int32, device="cuda")
    nb = int(L.pmgt_op_seg_sort_temp_bytes(M))
    k1, v1, sk, pm, off = mk(M), mk(M), mk(M), mk(M), mk(n_rows + 1)
    tmp = torch.empty(nb, dtype=torch.uint8, device="cuda")
    check(L.pmgt_op_seg_sort(P(ids_d), M, n_rows, P(k1), P(v1), P(sk), P(pm), P(off), P(tmp), nb, stream()))
    otdt = torch.float32 if out_code == 0 else torch.bfloat16
    out = nans((n_rows + 1, cols), otdt)
    part = nans((int(L.pmgt_op_seg_part_elems(M, cols)),))
    check(L.pmgt_op_seg_sum(in_code, out_code, P(src), src.stride(0), P(sk), P(pm), P(off), M, n_rows, cols, P(out), P(part), stream()))
    return out


@pytest.mark.parametrize("nf,d,Tq,S", [(2, 256, 24, 32), (3, 512, 10, 31), (4, 384, 6, 9)])
def test_table_mode_composition_equals_the_token_mode_reference(nf, d, Tq, S):
    """Table mode as the engine runs it (bf16): phase 1 forward per node -> phase 2 forward per token; phase 2 backward -> sort by node
    id -> segment sums (bf16 -> fp32) -> phase 1 backward.  The per-node dE and the summed partials of both phases equal the fp64
    reference of phase 0 on the gathered rows (dE summed per node), given the per-token dF the kernel wrote (bf16, itself checked against
    the fp64 dF).  Every stage is checked on its own as well: a and F_all per node, pre / h0 / stats per token, the segment sums."""
    L = H()
    tdt = torch.bfloat16
    M, n_rows = Tq * S, 53
    g = torch.Generator().manual_seed(d + nf)
    prm = _embed_params(nf, d, S + 3, g)
    dev = {k: v.cuda() for k, v in prm.items()}
    E = (torch.randn(n_rows, nf * d, generator=g) * 0.8).to(tdt)
    ids = torch.randint(2, n_rows - 1, (M,), generator=g)               # nodes 0, 1 and the last one unused: empty segments
    dh0 = torch.randn(M, d, generator=g).to(tdt)
    recompute = d == 256
    pe = L.pmgt_op_embed_part_elems(d, nf)
    Ed = E.cuda()
    a1, F_all = nans((n_rows, nf)), nans((n_rows, d), tdt)
    check(L.pmgt_op_embed_mix_fwd(C.byref(_embed_args("bf16", 1, n_rows, S, d, nf, E=Ed, a=a1, pre=F_all, **dev)), stream()))
    pre, stats, h0 = nans((M, d), tdt), nans((M, 2)), nans((M, d), tdt)
    t2 = dict(E=F_all, e_rows=ids.cuda(), pre=0 if recompute else pre, stats=stats, h0=h0, **dev)
    check(L.pmgt_op_embed_mix_fwd(C.byref(_embed_args("bf16", 2, M, S, d, nf, **t2)), stream()))
    dF, part2 = nans((M, d), tdt), nans((L.pmgt_op_embed_bwd_parts(M) * pe,))
    dh0d = dh0.cuda()
    check(L.pmgt_op_embed_mix_bwd(C.byref(_embed_args("bf16", 2, M, S, d, nf, dh0=dh0d, dF=dF, part=part2, **t2)), stream()))
    dFn = _seg_sum(ids.cuda(), dF, n_rows, 1, 0)
    dE, part1 = nans((n_rows, nf * d), tdt), nans((L.pmgt_op_embed_bwd_parts(n_rows) * pe,))
    check(L.pmgt_op_embed_mix_bwd(C.byref(_embed_args("bf16", 1, n_rows, S, d, nf, E=Ed, a=a1, dF=dFn, dF_f32=1, dE=dE, part=part1, **dev)),
                                  stream()))
    torch.cuda.synchronize()
    assert all_nan(dFn[n_rows:])
    # node phase forward: a and F_all against fp64 on the node rows
    r = {k: v.double().requires_grad_(True) for k, v in prm.items()}
    an, fn = _mix_ref(E.double(), r["Wa"], r["ba"], nf, d)
    assert_close(a1.cpu(), an, torch.float32, what="a (nodes)")
    assert_close(F_all.cpu(), fn, tdt, what="F_all")
    # token phase forward: x = F_all[id] + pos + role, from the F_all the kernel stored (bf16)
    s = torch.arange(M) % S
    Fk = F_all.cpu()[ids]
    if recompute:
        assert all_nan(pre)
        pre_k = ((Fk.float() + prm["pos"][s]) + prm["role"][(s > 0).long()]).to(tdt).double()
    else:
        pre_k = pre.double().cpu()
        assert_close(pre.cpu(), Fk.double() + prm["pos"].double()[s] + prm["role"].double()[(s > 0).long()], tdt, what="pre")
    # phase 0 on the gathered rows, the LayerNorm reading the kernel's sum
    Er = E.double()[ids].clone().requires_grad_(True)
    a, f = _mix_ref(Er, r["Wa"], r["ba"], nf, d)
    x, xs, st_ref, h = _token_ref(f, r, S, pre_k, torch.ones(M, d, dtype=torch.float64))
    assert_close(h0.cpu(), h, tdt, what="h0")
    assert_close(stats.cpu(), st_ref, torch.float32, what="stats")
    dF_ref, = torch.autograd.grad(h, xs, dh0.double(), retain_graph=True)
    assert_close(dF.cpu(), dF_ref, tdt, what="dF (tokens)")
    # the per-node sums of the per-token dF the kernel wrote; nodes 0, 1 and the last: empty segments, zero rows
    dFk = dF.double().cpu()
    sums = torch.zeros(n_rows, d, dtype=torch.float64).index_add_(0, ids, dFk)
    assert_close(dFn[:n_rows].cpu(), sums, torch.float32, floor=1e-6, what="segment sums")
    assert float(dFn[[0, 1, n_rows - 1]].abs().max()) == 0, "empty segments are zero rows"
    # backward of phase 0 per token from the same (bf16) per-token dF, summed per node: the node phase differentiates the mix once per
    # node with the summed dF (linear in dF, a and e depend on the node only), so both must agree
    xs.register_hook(lambda _: dFk)
    h.backward(dh0.double())
    dE_ref = torch.zeros(n_rows, nf * d, dtype=torch.float64).index_add_(0, ids, Er.grad)
    assert_close(dE.cpu(), dE_ref, tdt, what="dE per node")
    assert float(dE[[0, 1, n_rows - 1]].float().abs().max()) == 0
    p1, p2 = _reduce_parts(part1, n_rows, d, nf), _reduce_parts(part2, M, d, nf)
    assert float(p1["gamma"].abs().max()) == 0 and float(p2["Wa"].abs().max()) == 0
    assert_close(p2["gamma"].cpu(), r["gamma"].grad, torch.float32, what="dgamma")
    assert_close(p2["beta"].cpu(), r["beta"].grad, torch.float32, what="dbeta")
    assert_close(p1["Wa"].cpu(), r["Wa"].grad, torch.float32, what="dWa")
    assert_close(p1["ba"].cpu(), r["ba"].grad, torch.float32, what="dba")


@pytest.mark.parametrize("S,d,accumulate", [(9, 32, 0), (32, 256, 1), (64, 384, 0), (31, 1024, 1), (1, 256, 0)])
def test_pos_role_finish(S, d, accumulate):
    """dpos[s] = possum[s] for s < S and 0 up to max_pos (accumulate: +=, rows past S unchanged); drole = {possum[0], sum_{s>=1} possum[s]};
    rows past max_pos untouched."""
    L = H()
    g = torch.Generator().manual_seed(S * d)
    max_pos = S + 5
    possum = torch.randn(S, d, generator=g)
    dpos0 = torch.randn(max_pos, d, generator=g) if accumulate else torch.full((max_pos, d), NAN)
    drole0 = torch.randn(2, d, generator=g) if accumulate else torch.full((2, d), NAN)
    dpos = torch.cat([dpos0, torch.full((2, d), NAN)]).cuda()
    drole = torch.cat([drole0, torch.full((1, d), NAN)]).cuda()
    possum_d = possum.cuda()
    check(L.pmgt_op_pos_role_finish(P(possum_d), S, d, max_pos, P(dpos), P(drole), accumulate, stream()))
    torch.cuda.synchronize()
    dpos, drole = dpos.cpu(), drole.cpu()
    want = possum + dpos0[:S] if accumulate else possum
    assert torch.equal(dpos[:S], want)
    assert torch.equal(dpos[S:max_pos], dpos0[S:] if accumulate else torch.zeros(max_pos - S, d))
    assert all_nan(dpos[max_pos:]) and all_nan(drole[2:])
    assert torch.equal(drole[0], possum[0] + drole0[0] if accumulate else possum[0])
    r1 = possum[1:].double().sum(0) + (drole0[1].double() if accumulate else 0)
    assert_close(drole[1], r1, torch.float32, floor=1e-6, what="drole[1]")


# =========================================================================================== segment sums
def _seg_ids(M, n_rows, layout, rs):
    if layout == "uniform":
        ids = rs.randint(0, n_rows, M)
    elif layout == "half":                     # one id holds half the tokens
        ids = rs.randint(0, n_rows, M)
        ids[rs.permutation(M)[: M // 2]] = n_rows // 2
    elif layout == "chunks64":                 # every used id holds exactly 64 tokens: the sorted segments are the chunks
        assert M % 64 == 0 and n_rows >= M // 64
        ids = np.repeat(rs.permutation(n_rows)[: M // 64], 64)
    elif layout == "spanning":                 # segments of 1 .. 200 tokens starting mid-chunk, gaps (empty ids), ids 0 and last empty
        out, nid = [], 1
        while len(out) < M:
            out += [nid] * int(rs.randint(1, 201))
            nid += 1 + int(rs.randint(0, 2))
        assert nid < n_rows - 1
        ids = np.array(out[:M])
    else:                                      # "empty_ends": ids 0 and n_rows - 1 never occur
        ids = rs.randint(1, n_rows - 1, M)
    return rs.permutation(ids).astype(np.int64)


SEG_CASES = [
    # M, n_rows, layout, cols, ld
    (1, 1, "uniform", 4, 4),
    (1, 3, "empty_ends", 252, 256),
    (63, 3, "uniform", 256, 260),
    (64, 1, "uniform", 260, 260),
    (65, 3, "half", 512, 516),
    (65, 40, "empty_ends", 1020, 1024),
    (4097, 40, "half", 1024, 1024),
    (4097, 7254, "spanning", 260, 264),
    (4096, 64, "chunks64", 256, 256),
    (4097, 3, "uniform", 4, 8),
    (4097, 7254, "uniform", 1020, 1020),
    (393216, 7254, "half", 256, 256),          # the bench's C2 token count
    (393216, 7254, "spanning", 512, 512),
    (393216, 7254, "chunks64", 256, 260),
]
SEG_DT = [(0, 0), (1, 1), (1, 0)]              # (in, out): fp32 -> fp32, bf16 -> bf16, bf16 -> fp32


@pytest.mark.parametrize("io", SEG_DT, ids=["f32f32", "bf16bf16", "bf16f32"])
@pytest.mark.parametrize("M,n_rows,layout,cols,ld", SEG_CASES)
def test_segment_sums_are_exact_on_integer_rows(M, n_rows, layout, cols, ld, io):
    """seg_sum + seg_fix (segsum.hip) after seg_sort: integer-valued rows make every fp32 sum exact, so a wrong, missed or doubled row
    shows as a bit difference.  Columns between cols and the row stride ld hold NaN and must not leak in; bf16 output = the exact sum
    rounded to nearest even."""
    rs = np.random.RandomState(M % 977 + n_rows + cols)
    ids = _seg_ids(M, n_rows, layout, rs)
    tdt = torch.float32 if io[0] == 0 else torch.bfloat16
    src = torch.randint(-8, 9, (M, ld), device="cuda").to(tdt)
    src[:, cols:] = NAN
    ids_d = torch.from_numpy(ids).cuda()
    out = _seg_sum(ids_d, src, n_rows, io[0], io[1], cols)
    ref = torch.zeros(n_rows, cols, dtype=torch.float64, device="cuda").index_add_(0, ids_d, src[:, :cols].double())
    torch.cuda.synchronize()
    assert all_nan(out[n_rows:])
    want = ref.float() if io[1] == 0 else ref.to(torch.bfloat16)
    same = out[:n_rows] == want
    assert bool(same.all()), f"{int((~same).sum())} elements differ; first rows {torch.nonzero(~same)[:4, 0].tolist()}"


# =========================================================================================== GSR
def _gsr_ref(cls, B, npairs, labels):
    """oracle gsr_loss on the CLS rows (targets, then pairs), fp64 with autograd: logits, loss_i / B, d loss / d cls"""
    cls = cls.clone().requires_grad_(True)
    zt, zp = Fn.normalize(cls[:B], dim=-1), Fn.normalize(cls[B:], dim=-1)
    owner = torch.repeat_interleave(torch.arange(B, device=cls.device), npairs)
    logits = (zp * zt[owner]).sum(-1)
    per = Fn.binary_cross_entropy_with_logits(logits, labels, reduction="none")
    part = torch.zeros(B, dtype=per.dtype, device=per.device).index_add_(0, owner, per) / npairs.double() / B
    part.sum().backward()
    return logits.detach(), part.detach(), cls.grad


GSR_CASES = [
    # dt, B, d, layout, S
    ("fp32", 1, 32, "full", 9),
    ("bf16", 3, 128, "full", 9),
    ("fp32", 5, 384, "full", 4),
    ("bf16", 5, 1024, "compact", 0),
    ("fp32", 1024, 256, "full", 3),
    ("bf16", 1024, 512, "compact", 0),
    ("bf16", 4096, 256, "compact", 0),
    ("fp32", 4096, 128, "compact", 0),
    ("fp32", 3, 1024, "full", 9),
    ("bf16", 64, 384, "full", 2),
]


@pytest.mark.parametrize("dt,B,d,layout,S", GSR_CASES)
def test_gsr_loss_logits_and_cls_gradients(dt, B, d, layout, S):
    """gsr_kernel: cosine logits, per-target mean BCE / B and the gradient on the CLS rows, full layout (CLS rows S d apart) and compacted
    (cls_stride = d, rows of the masked tokens behind), pair counts 1 .. 70 per target (crossing a wave of 64).  Non-CLS rows of dh and
    the rows behind the compacted CLS block stay NaN.  One target row and one pair row of norm 0 in the small cases (F.normalize's clamp)."""
    L = H()
    code, tdt = DT[dt]
    g = torch.Generator().manual_seed(B * 7 + d)
    npairs = torch.randint(1, 71, (B,), generator=g)
    for i, v in enumerate((64, 65, 1, 70, 63)):
        if i < B:
            npairs[i] = v
    Pn = int(npairs.sum())
    rows = B + Pn
    cls = torch.randn(rows, d, generator=g) * 0.7
    if B <= 5:
        cls[B - 1] = 0
        cls[B + 2] = 0
    cls = cls.to(tdt)
    labels = (torch.rand(Pn, generator=g) < 0.5).float()
    if layout == "full":
        h = torch.randn(rows * S, d, generator=g).to(tdt)
        h.view(rows, S, d)[:, 0] = cls
        stride = S * d
    else:
        h = torch.cat([cls, torch.randn(37, d, generator=g).to(tdt)])
        stride = d
    hd = h.cuda()
    dh = nans(tuple(h.shape), tdt)
    off = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(npairs, 0)]).int().cuda()
    logits, lpart = nans((Pn + 1,)), nans((B + 1,))
    lab = labels.cuda()
    check(L.pmgt_op_gsr(code, P(hd), P(dh), B, S, d, stride, P(off), P(lab), P(logits), P(lpart), stream()))
    lg, lp, gr = _gsr_ref(cls.double().cuda(), B, npairs.cuda(), labels.double().cuda())
    torch.cuda.synchronize()
    f32 = torch.float32
    assert_close(logits[:Pn], lg, f32, floor=1e-5, what="logits")
    assert_close(lpart[:B], lp, f32, floor=1e-5, what="loss parts")
    assert all_nan(logits[Pn:]) and all_nan(lpart[B:])
    if layout == "full":
        dcls = dh.view(rows, S, d)[:, 0]
        assert all_nan(dh.view(rows, S, d)[:, 1:]), "non-CLS rows of dh"
    else:
        dcls = dh[:rows]
        assert all_nan(dh[rows:]), "rows behind the compacted CLS block"
    zero = cls.float().abs().sum(1).cuda() == 0        # judged on their own: their gradient is ~1e12 times the others'
    assert_close(dcls[~zero], gr[~zero], tdt, what="dh (CLS rows)")
    assert_close(dcls[zero], gr[zero], tdt, what="dh (CLS rows of norm 0)")
    # evaluation form: dh == NULL writes logits and loss parts only
    logits2, lpart2 = nans((Pn,)), nans((B,))
    check(L.pmgt_op_gsr(code, P(hd), None, B, S, d, stride, P(off), P(lab), P(logits2), P(lpart2), stream()))
    torch.cuda.synchronize()
    assert torch.equal(logits2, logits[:Pn]) and torch.equal(lpart2, lpart[:B])


# =========================================================================================== NFR + loss_finish
NFR_B, NFR_S = 1024, 32
CAP = NFR_B * (NFR_S - 1)
NFR_CASES = ([("bf16", (1536, 768), n, False) for n in (0, 1, 7, 8, 9, CAP - 1, CAP)]
             + [("bf16", (64, 128, 32, 256), n, False) for n in (0, 1, 7, 8, 9, CAP - 1, CAP)]
             + [("bf16", (768,), n, False) for n in (0, 8, CAP)]
             + [("bf16", (1536, 768, 256), n, False) for n in (1, 9, CAP - 1)]
             + [("fp32", f, n, False) for f in ((768,), (64, 128, 32, 256), (1536, 768, 256)) for n in (0, 9, CAP)]
             + [("bf16", (1536, 768), n, True) for n in (1, 9, CAP)]
             + [("bf16", (64, 128, 32, 256), n, True) for n in (7, CAP - 1)])


@pytest.mark.parametrize("dt,feats,n,f8", NFR_CASES)
def test_nfr_diff_and_loss_finish(dt, feats, n, f8):
    """nfr_diff_kernel: dpred = (2 / nf) (pred - target) / (n F_f) per modality for the n live rows (rows at or past n untouched), squared
    errors per modality into the partials (unused partials zero); loss_finish: {gsr + nfr, gsr, nfr} with nfr = mean_f sse_f / (n F_f),
    NaN for n = 0 (quirk Q2), and the count copied out.  e4m3 tables: targets are the dequantised bytes times the table's scale."""
    L = H()
    code, tdt = DT[dt]
    nf, Ftot = len(feats), sum(feats)
    g = torch.Generator().manual_seed(n + Ftot + nf + (7 if f8 else 0))
    N = 5000
    tables, deq, scales = [], [], []
    for Fm in feats:
        if f8:
            b = torch.randint(0, 256, (N + 2, Fm), generator=g, dtype=torch.int32).to(torch.uint8)
            b[(b & 0x7F) == 0x7F] = 0x3C                              # no NaN encodings
            sc = 0.01 * (1 + len(scales))
            tables.append(b.cuda())
            deq.append(b.view(torch.float8_e4m3fn).cuda().double() * sc)
            scales.append(sc)
        else:
            t = torch.randn(N + 2, Fm, generator=g).to(tdt)
            tables.append(t.cuda())
            deq.append(t.cuda().double())
            scales.append(1.0)
    tids = torch.randint(0, N + 2, (CAP,), generator=g)
    pred0 = (torch.randn(CAP, Ftot, generator=g) * 1.5).to(tdt)
    pred0[n:] = NAN
    pred = pred0.cuda()
    cnt = torch.tensor([n], dtype=torch.int32, device="cuda")
    parts = L.pmgt_op_nfr_diff_parts(CAP)
    sse = nans((parts + 1, 4))
    Fa = (C.c_int * nf)(*feats)
    Ta = (C.c_void_p * nf)(*[t.data_ptr() for t in tables])
    Sa = (C.c_float * nf)(*scales)
    tids_d = tids.cuda()
    check(L.pmgt_op_nfr_diff(code, P(pred), P(tids_d), P(cnt), CAP, nf, Fa, Ta, int(f8), Sa, P(sse), stream()))
    gsr_part = torch.randn(NFR_B, generator=g).cuda() * 1e-3
    out, cout = nans((4,)), torch.full((2,), -7, dtype=torch.int32, device="cuda")
    check(L.pmgt_op_loss_finish(P(gsr_part), NFR_B, P(sse), parts, P(cnt), nf, Fa, 1, P(out), P(cout), stream()))
    torch.cuda.synchronize()
    assert all_nan(pred[n:]), "rows at or past the live count"
    assert all_nan(sse[parts:])
    used = (n + 7) // 8
    if used < parts:
        assert float(sse[used:parts].abs().max()) == 0, "partials of blocks past the live count"
    if nf < 4:
        assert float(sse[:parts, nf:].abs().max()) == 0, "modalities past nf"
    # reference
    tg = torch.cat([dq[tids_d[:n]] for dq in deq], 1)
    diff = pred0[:n].double().cuda() - tg
    col_f = torch.cat([torch.full((Fm,), i, dtype=torch.int64) for i, Fm in enumerate(feats)]).cuda()
    Fcol = torch.tensor(feats, dtype=torch.float64, device="cuda")[col_f]
    if n:
        assert_close(pred[:n], (2.0 / nf) * diff / (n * Fcol), tdt, what="dpred")
    sse_ref = torch.stack([(diff[:, col_f == i] ** 2).sum() for i in range(nf)])
    assert_close(sse[:used, :nf].double().sum(0), sse_ref, torch.float32, floor=1e-5, what="sse")
    gsr = float(gsr_part.double().sum())
    gabs = float(gsr_part.abs().sum())
    out = out.cpu().double()
    assert abs(float(out[1]) - gsr) <= 1e-5 * gabs
    assert int(cout[0]) == n and int(cout[1]) == -7 and all_nan(out[3:])
    if n == 0:
        assert math.isnan(float(out[2])) and math.isnan(float(out[0])), "an empty mask gives a NaN NFR term and total (quirk Q2)"
    else:
        nfr = float((sse_ref / (n * torch.tensor(feats, dtype=torch.float64, device="cuda"))).mean())
        assert abs(float(out[2]) - nfr) <= 1e-5 * nfr
        assert abs(float(out[0]) - (nfr + gsr)) <= 1e-5 * (nfr + gabs)


def test_loss_finish_without_nfr():
    """evaluation: with_nfr = 0 -> {gsr, gsr, 0}; the count is neither read nor copied"""
    L = H()
    B = 1025
    gp = torch.randn(B, device="cuda")
    out, cout = nans((3,)), torch.full((1,), -7, dtype=torch.int32, device="cuda")
    Fa = (C.c_int * 2)(768, 1536)
    check(L.pmgt_op_loss_finish(P(gp), B, None, 0, None, 2, Fa, 0, P(out), P(cout), stream()))
    torch.cuda.synchronize()
    s = float(gp.double().sum())
    assert abs(float(out[1]) - s) <= 1e-5 * float(gp.abs().sum()) and float(out[0]) == float(out[1]) and float(out[2]) == 0
    assert int(cout[0]) == -7


# =========================================================================================== integer bookkeeping
@pytest.mark.parametrize("B", [1, 1023, 1024, 1025, 4096])
def test_pair_offsets_is_the_exclusive_cumsum(B):
    """pair_offsets_kernel: one 1024-thread block, several targets per thread past B = 1024"""
    L = H()
    g = torch.Generator().manual_seed(B)
    npairs = torch.randint(0, 71, (B,), generator=g)
    off = torch.full((B + 2,), -7, dtype=torch.int32, device="cuda")
    npairs_d = npairs.cuda()
    check(L.pmgt_op_pair_offsets(P(npairs_d), B, P(off), stream()))
    torch.cuda.synchronize()
    want = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(npairs, 0)])
    assert torch.equal(off[:B + 1].cpu().long(), want) and int(off[B + 1]) == -7


@pytest.mark.parametrize("seq_off", [0, 37])
@pytest.mark.parametrize("density", [0.0, "one", 0.16, 1.0])
@pytest.mark.parametrize("B", [1, 1023, 1024, 1025, 4096])
def test_nfr_compact_is_the_row_major_nonzero_order(B, density, seq_off):
    """nfr_compact_kernel (ballot ranks over slabs of 1024 positions): rows / tids of the masked positions in row-major order, the count;
    entries past the count untouched"""
    L = H()
    S = 32 if B % 2 == 0 else 9
    g = torch.Generator().manual_seed(B + S)
    n = B * S
    if density == "one":
        hit = torch.zeros(n, dtype=torch.bool)
        hit[int(torch.randint(0, n, (1,), generator=g))] = True
    else:
        hit = torch.rand(n, generator=g) < density
    tgt = torch.where(hit, torch.randint(0, 10 ** 6, (n,), generator=g), torch.full((n,), -1, dtype=torch.int64))
    rows, tids = (torch.full((n + 1,), -7, dtype=torch.int64, device="cuda") for _ in range(2))
    cnt = torch.full((2,), -7, dtype=torch.int32, device="cuda")
    tgt_d = tgt.cuda()
    check(L.pmgt_op_nfr_compact(P(tgt_d), B, S, seq_off, P(rows), P(tids), P(cnt), stream()))
    torch.cuda.synchronize()
    idx = torch.nonzero(hit).flatten()
    k = idx.numel()
    assert int(cnt[0]) == k and int(cnt[1]) == -7
    assert torch.equal(rows[:k].cpu(), seq_off * S + idx) and torch.equal(tids[:k].cpu(), tgt[idx])
    assert bool((rows[k:] == -7).all()) and bool((tids[k:] == -7).all())


@pytest.mark.parametrize("dt,cap,count,d,add", [("fp32", 1, 1, 4, 0), ("bf16", 100, 37, 256, 0), ("bf16", 100, 100, 260, 1),
                                                ("fp32", 5000, 4999, 1024, 1), ("bf16", 150000, 149999, 256, 1), ("fp32", 64, 0, 256, 0)])
def test_scatter_rows_copies_and_adds(dt, cap, count, d, add):
    """scatter_rows_kernel: dst[rows[k]] = src[k] (add: dst + src, one rounding) for k < count; every other row of dst untouched"""
    L = H()
    code, tdt = DT[dt]
    g = torch.Generator().manual_seed(cap + d)
    n_dst = cap + 50
    rows = torch.randperm(n_dst, generator=g)[:cap]
    src = torch.randn(cap, d, generator=g).to(tdt)
    dst0 = torch.randn(n_dst, d, generator=g).to(tdt) if add else torch.full((n_dst, d), NAN).to(tdt)
    dst = dst0.cuda()
    cnt = torch.tensor([count], dtype=torch.int32, device="cuda")
    src_d, rows_d = src.cuda(), rows.cuda()
    check(L.pmgt_op_scatter_rows(code, P(src_d), P(rows_d), P(cnt), cap, d, P(dst), add, stream()))
    torch.cuda.synchronize()
    want = dst0.clone()
    r = rows[:count]
    want[r] = (dst0[r].float() + src[:count].float()).to(tdt) if add else src[:count]
    got = dst.cpu()
    assert torch.equal(torch.isnan(got.float()), torch.isnan(want.float()))
    assert torch.equal(torch.nan_to_num(got.float()), torch.nan_to_num(want.float()))


# =========================================================================================== clip + AdamW
ADAM = {k: float(np.float32(v)) for k, v in dict(lr=1e-3, wd=0.01, b1=0.9, b2=0.999, eps=1e-8).items()}    # as the kernel receives them


def _adamw(p, g, m, v, dec, n, max_norm, step, scal, part):
    a = ADAM
    check(H().pmgt_op_adamw(P(p), P(g), P(m), P(v), P(dec), n, a["lr"], a["wd"], a["b1"], a["b2"], a["eps"], max_norm, P(step), P(scal),
                            P(part), stream()))


@pytest.mark.parametrize("mode", ["off", "inactive", "active"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 4095, 1 << 20, (1 << 22) + 3])
def test_clip_and_adamw_three_steps(n, mode):
    """sqnorm_part (grid-stride over up to 1024 blocks + scalar tail) -> adam_prepare (step counter, clip coefficient, bias corrections on
    the device) -> adamw, three consecutive steps with m, v, step and scal kept on the device.  Each step is compared with the fp64
    restatement of clip_grad_norm + adamw_step applied to the kernel's state before it (with the kernel's clip coefficient, itself checked
    against the fp64 one); p within 2 ulp + 1e-3 lr (one step moves p by about lr)."""
    a = ADAM
    gen = torch.Generator(device="cuda").manual_seed(n)
    p = torch.randn(n, device="cuda", generator=gen)
    m, v = torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    dec = (torch.rand(n, device="cuda", generator=gen) < 0.6).to(torch.uint8)
    step = torch.zeros(1, dtype=torch.int64, device="cuda")
    scal, part = nans((4,)), nans((1024,))
    for t in (1, 2, 3):
        g = torch.randn(n, device="cuda", generator=gen) * (0.5 * t)
        norm = float(g.double().norm())
        max_norm = {"off": 0.0, "inactive": 10.0 * norm + 1.0, "active": 0.01 * norm}[mode]
        p0, m0, v0 = p.double(), m.double(), v.double()
        _adamw(p, g, m, v, dec, n, max_norm, step, scal, part)
        torch.cuda.synchronize()
        coef = min(max_norm / (norm + 1e-6), 1.0) if max_norm > 0 else 1.0
        bc1, bc2 = 1 - a["b1"] ** t, 1 - a["b2"] ** t
        assert int(step[0]) == t
        sc = scal.cpu().double()
        assert abs(float(sc[3]) - norm) <= 1e-5 * norm
        assert abs(float(sc[0]) - coef) <= 1e-5 * coef
        if mode == "active":
            assert float(sc[0]) < 0.02
        else:
            assert float(sc[0]) == 1.0
        assert abs(float(sc[1]) - a["lr"] / bc1) <= 1e-6 * a["lr"] / bc1
        assert abs(float(sc[2]) - 1 / math.sqrt(bc2)) <= 1e-6 / math.sqrt(bc2)
        gg = g.double() * float(sc[0])
        m_ref = a["b1"] * m0 + (1 - a["b1"]) * gg
        v_ref = a["b2"] * v0 + (1 - a["b2"]) * gg * gg
        p_ref = p0 * (1 - a["lr"] * a["wd"] * dec.double()) - (a["lr"] / bc1) * m_ref / (v_ref.sqrt() / math.sqrt(bc2) + a["eps"])
        assert_close(m, m_ref, torch.float32, ulps=16, floor=1e-7, what=f"m (step {t})")
        assert_close(v, v_ref, torch.float32, ulps=16, floor=1e-7, what=f"v (step {t})")
        err = (p.double() - p_ref).abs()
        bound = 2 * ulp(p_ref, torch.float32) + 1e-3 * a["lr"]
        assert bool((err <= bound).all()), f"p (step {t}): max error {float(err.max())!r}, {int((err > bound).sum())} elements out of bound"


@pytest.mark.parametrize("n", [4095, 1 << 20])
def test_adamw_zero_gradients_only_decay(n):
    """g = 0: the norm is 0 (coefficient 1 even with clipping on), m and v stay exactly 0, p only decays where the mask says so"""
    a = ADAM
    gen = torch.Generator(device="cuda").manual_seed(n + 1)
    p = torch.randn(n, device="cuda", generator=gen)
    p0 = p.clone()
    g, m, v = (torch.zeros(n, device="cuda") for _ in range(3))
    dec = (torch.rand(n, device="cuda", generator=gen) < 0.5).to(torch.uint8)
    step = torch.full((1,), 4, dtype=torch.int64, device="cuda")
    scal, part = nans((4,)), nans((1024,))
    _adamw(p, g, m, v, dec, n, 1.0, step, scal, part)
    torch.cuda.synchronize()
    assert int(step[0]) == 5 and float(scal[3]) == 0 and float(scal[0]) == 1
    assert bool((m == 0).all()) and bool((v == 0).all())
    ref = p0.double() * (1 - a["lr"] * a["wd"] * dec.double())
    assert bool(((p.double() - ref).abs() <= 2 * ulp(ref, torch.float32)).all())
    assert torch.equal(p[dec == 0], p0[dec == 0])


# =========================================================================================== weight mirror
def _to_head_major(t, Hh, dh):
    """[..., 4d] in q | k | v | c column order -> head-major (h, matrix, w)  (as test_ops_gpu._to_head_major)"""
    lead = t.shape[:-1]
    return t.reshape(*lead, 4, Hh, dh).transpose(-3, -2).reshape(*lead, 4 * Hh * dh).contiguous()


@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("variant", ["all", "transposes_only"])
def test_mirror_copies_transposes_and_head_major(dt, variant):
    """mirror_kernel with several descriptors in one launch (tile_start boundaries crossed): same-layout copies and transposes of
    (1, 1), (33, 31), (256, 256), (2304, 256), (1024, 256) and head-major transposes of Q|K|V|C weights [4d, d] (d in {128, 256}, head
    sizes 32 / 64), bit-equal to torch's round-to-nearest-even cast; every element of the mirror outside the written regions stays NaN."""
    L = H()
    code, tdt = DT[dt]
    bits = torch.int16 if tdt == torch.bfloat16 else torch.int32
    g = torch.Generator().manual_seed(11)
    plain = [(1, 1), (33, 31), (256, 256), (2304, 256), (1024, 256)]
    hm = [(128, 32), (256, 64), (256, 32), (128, 64)]
    shapes = [(r, c, 0, 0) for r, c in plain] + [(4 * d, d, d, dh) for d, dh in hm]
    params, descs, expect = [], [], []
    poff, moff, tiles = 0, 0, 0
    for k, (r, c, hd, hdh) in enumerate(shapes):
        W = torch.randn(r, c, generator=g) * 3
        poff += 3
        params.append((poff, W))
        dd = _lib().MirrorDescC()
        dd.src, dd.rows, dd.cols, dd.hm_d, dd.hm_dh, dd.tile_start = poff, r, c, hd, hdh, tiles
        poff += r * c
        tiles += ((r + 31) // 32) * ((c + 31) // 32)
        on = {"dst": variant == "all" and k % 2 == 0, "dst_t": variant != "all" or k % 3 != 1, "dst_t_hm": hd > 0}
        regions = {}
        for key in ("dst", "dst_t", "dst_t_hm"):
            if on[key]:
                moff += 5
                regions[key] = moff
                moff += r * c
            setattr(dd, key, regions.get(key, -1))
        descs.append(dd)
        Wc = W.to(tdt)
        if "dst" in regions:
            expect.append((regions["dst"], Wc.flatten()))
        if "dst_t" in regions:
            expect.append((regions["dst_t"], Wc.T.contiguous().flatten()))
        if "dst_t_hm" in regions:
            expect.append((regions["dst_t_hm"], _to_head_major(Wc.T.contiguous(), hd // hdh, hdh).flatten()))
    flat = torch.full((poff + 7,), NAN)
    for o, W in params:
        flat[o:o + W.numel()] = W.flatten()
    mirror = nans((moff + 9,), tdt)
    arr = (_lib().MirrorDescC * len(descs))(*descs)
    flat_d = flat.cuda()
    check(L.pmgt_op_mirror(code, P(flat_d), P(mirror), arr, len(descs), tiles, stream()))
    torch.cuda.synchronize()
    got = mirror.cpu()
    written = torch.zeros(got.numel(), dtype=torch.bool)
    for o, want in expect:
        seg = got[o:o + want.numel()]
        assert torch.equal(seg.view(bits), want.view(bits)), f"region at {o}"
        written[o:o + want.numel()] = True
    assert all_nan(got[~written]), "elements outside every written region"
