"""Every dropout-bearing kernel, run through its pmgt_op_* entry with drop_p > 0, against a plain fp64 torch computation that multiplies
by keep(...) / (1 - p) where the reference does (transformers 4.11.2 BertSelfOutput / BertOutput: dense -> dropout -> + residual ->
LayerNorm; pmgt/pmgt/modeling_pmgt.py:458,513: each softmax branch before the beta mix; :207-208: after the embedding LayerNorm).
The masks come from tests/dropout_util.py, the numpy restatement of the kernels' counter hash that test_dropout_rng_gpu.py pins to the
device bit for bit -- so VALUES are compared, not only sibling kernels that share the hash and the indexing idiom.

Tolerances are the project's own for the same kernel with dropout off (tol(dt) and the per-test bounds of test_ops_gpu.py /
test_rowops_gpu.py): dropout zeroes values and rescales the survivors, which leaves a relative error unchanged.  Where a zero pattern is
compared it is compared exactly; the only elements whose zero is not the mask's are named (masked-key columns of the probabilities)."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from tests import dropout_util as du
from tests.test_ops_gpu import DT, P, _from_head_major, _setup, _to_head_major, rel_err, rounded, stream, to_dev, tol

pytestmark = pytest.mark.gpu

SEED, STEP = (1 << 32) + 99, 3


def rng_t():
    return torch.tensor([SEED, STEP], dtype=torch.int64, device="cuda")


def keep_t(site, rows, cols, p, device="cpu"):
    """fp64 multiplier keep / (1 - p) of site `site` at (SEED, STEP), and the boolean mask."""
    k = torch.from_numpy(du.keep(SEED, STEP, site, rows, cols, p)).to(device)
    return k.double() / (1.0 - float(np.float32(p))), k


DENSE_FAMILIES = ("gemm_ws", "gemm_wsr", "gemm_wsr512", "gemm_rowln", "nt_lnf", "nt_big", "nt_big_128", "nt_tile")


def _trace(H):
    return {f: int(H.pmgt_launch_trace_count(f.encode())) for f in DENSE_FAMILIES}


# ------------------------------------------------------------------------------------------- dense epilogues
@pytest.mark.parametrize("entry,dt,M,N,K,ln,family", [
    ("linear", "bf16", 4096, 256, 256, True, "gemm_ws"),         # attn-out / FFN2 shape below the role-split form
    ("linear", "bf16", 640, 128, 128, False, "gemm_ws"),
    ("linear", "bf16", 9000, 256, 256, True, "gemm_wsr"),        # ragged M
    ("linear", "bf16", 8193, 256, 256, True, "gemm_wsr"),        # one row in the last tile
    ("linear", "bf16", 9001, 512, 512, False, "gemm_wsr512"),
    ("linear", "bf16", 5000, 512, 512, True, "gemm_rowln"),
    ("linear", "bf16", 4097, 512, 512, True, "gemm_rowln"),      # one row in the last tile
    ("linear", "bf16", 24577, 256, 1024, True, "nt_lnf"),        # one row in the last tile
    ("gemm_nt", "bf16", 24577, 256, 1024, False, "nt_big"),
    ("gemm_nt", "bf16", 24600, 128, 256, False, "nt_big_128"),   # N % 256 != 0: the 256 x 128 variant
    ("gemm_nt", "bf16", 333, 136, 72, False, "nt_tile"),
    ("gemm_nt", "fp32", 333, 136, 96, False, "nt_tile"),
    ("gemm_nt", "fp32", 77, 40, 24, False, "nt_tile"),
    ("linear", "bf16", 100, 264, 256, False, "gemm_ws"),         # N not a multiple of the 256-column slab
    ("linear", "bf16", 777, 256, 256, True, "nt_tile"),          # option tile_gemm: the tiled kernel + a LayerNorm launch
])
def test_dense_epilogue_dropout_values_match_fp64_with_restated_masks(entry, dt, M, N, K, ln, family):
    """C = dropout(A W^T + b) + residual: dropout on the dense output BEFORE the residual; where the fused form computes them, the
    LayerNorm of the (storage-rounded) sum and its {mean, rstd}.  The launch trace must show exactly the family the case is for.  A second
    run with a zero residual gives the exact zero pattern: C == 0 exactly where the restated mask drops (random normal operands: no
    element is left out)."""
    _lib, L = _setup()
    H = _lib.hip()
    code, tdt = DT[dt]
    p, site = 0.1, du.site_id(2, du.SITE_FO)
    g = torch.Generator().manual_seed(M + N + K)
    A = to_dev(torch.randn(M, K, generator=g), tdt)
    W = to_dev(torch.randn(N, K, generator=g) * 0.2, tdt)
    bias = torch.randn(N, generator=g).cuda()
    R = to_dev(torch.randn(M, N, generator=g), tdt)
    gam = (1 + 0.1 * torch.randn(N, generator=g)).cuda()
    bet = (0.1 * torch.randn(N, generator=g)).cuda()
    rng = rng_t()
    km, kb = keep_t(site, M, N, p, "cuda")
    pre = A.double() @ W.double().T + bias.double()
    L.use(*(["tile_gemm"] if (entry, family) == ("linear", "nt_tile") else []))

    def run(res):
        Cd = torch.full((M, N), float("nan"), device="cuda", dtype=tdt)
        lno = torch.full((M, N), float("nan"), device="cuda", dtype=tdt) if ln else None
        stats = torch.full((M, 2), float("nan"), device="cuda") if ln else None
        H.pmgt_launch_trace_reset()
        if entry == "linear":
            _lib.check(L.pmgt_op_linear(code, P(A), K, P(W), K, P(Cd), N, M, N, K, P(bias), 0, None, N, P(res), N, p, site, P(rng),
                                        P(lno), P(stats), P(gam) if ln else None, P(bet) if ln else None, 1e-12, stream()))
        else:
            _lib.check(L.pmgt_op_gemm_nt(code, P(A), K, None, P(W), K, P(Cd), N, M, N, K, P(bias), 0, None, 0, P(res), N, p, site,
                                         P(rng), None, stream()))
        torch.cuda.synchronize()
        tr = _trace(H)
        assert tr[family] == 1 and sum(tr.values()) == 1, (family, tr)
        return Cd, lno, stats

    Cd, lno, stats = run(R)
    ref = pre * km + R.double()
    e = {"C": rel_err(Cd, ref)}
    assert e["C"] < tol(dt), e
    if ln:
        x = ref.to(tdt).double()           # gemm.h: ln_out = LN(C) with C the storage-rounded epilogue result
        lref = torch.nn.functional.layer_norm(x, (N,), gam.double(), bet.double(), 1e-12)
        sref = torch.stack([x.mean(1), 1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-12)], 1)
        e["ln"], e["stats"] = rel_err(lno, lref), rel_err(stats, sref)
        assert e["ln"] < 2e-2 and e["stats"] < 1e-3, e
    Z = torch.zeros_like(R)
    C0, _, _ = run(Z)
    L.use()
    assert torch.equal(C0 == 0, ~kb), int(((C0 == 0) != ~kb).sum())
    e["C0"] = rel_err(C0, pre * km)
    assert e["C0"] < tol(dt), e
    print(f"dense dropout {family} {dt} {M}x{N}x{K}: {e}")


# ------------------------------------------------------------------------------------------- LayerNorm forward / backward
@pytest.mark.parametrize("dt", ["fp32", "bf16"])
@pytest.mark.parametrize("M,d", [(100, 64), (257, 256), (64, 512), (33, 1024), (10, 128)])
def test_layernorm_dropout_masks_forward_and_backward(dt, M, d):
    """y = dropout_in(LN(x)) (the embedding's form); backward: dy passes the same input-side mask, dx_drop = dropout_out(dx) (the mask
    of the dense layer in front), dgb = dgamma | dbeta | column sums of dx_drop."""
    _lib, L = _setup()
    code, tdt = DT[dt]
    p_in, p_out, s_in, s_out = 0.1, 0.25, du.site_id(-1, du.SITE_EMB), du.site_id(1, du.SITE_AO)
    g = torch.Generator().manual_seed(d + 1)
    x = torch.randn(M, d, generator=g) * 2 + 0.5
    gam = 1 + 0.1 * torch.randn(d, generator=g)
    bet = 0.1 * torch.randn(d, generator=g)
    dy = torch.randn(M, d, generator=g)
    xd, gd, bd, dyd = to_dev(x, tdt), gam.cuda(), bet.cuda(), to_dev(dy, tdt)
    rng = rng_t()
    y = torch.full((M, d), float("nan"), device="cuda", dtype=tdt)
    stats = torch.empty(M, 2, device="cuda")
    _lib.check(L.pmgt_op_layernorm_fwd(code, P(xd), P(y), P(stats), P(gd), P(bd), M, d, 1e-12, p_in, s_in, P(rng), stream()))
    k_in, kb_in = keep_t(s_in, M, d, p_in)
    k_out, kb_out = keep_t(s_out, M, d, p_out)
    xr = rounded(x, tdt).requires_grad_(True)
    gr, br = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(xr, (d,), gr, br, 1e-12) * k_in
    assert torch.equal((y == 0).cpu(), ~kb_in)
    assert rel_err(y, ref.detach()) < tol(dt)
    ref.backward(rounded(dy, tdt))
    dx = torch.full((M, d), float("nan"), device="cuda", dtype=tdt)
    dxd = torch.full((M, d), float("nan"), device="cuda", dtype=tdt)
    part = torch.empty(((M + 63) // 64) * 3 * d, device="cuda")
    dgb = torch.empty(3 * d, device="cuda")
    _lib.check(L.pmgt_op_layernorm_bwd(code, P(dyd), P(xd), P(stats), P(gd), P(dx), P(dxd), P(part), P(dgb), M, d, p_in, s_in, p_out, s_out,
                                       P(rng), stream()))
    e = dict(dx=rel_err(dx, xr.grad), dxd=rel_err(dxd, xr.grad * k_out), dgamma=rel_err(dgb[:d], gr.grad), dbeta=rel_err(dgb[d:2 * d], br.grad),
             colsum=rel_err(dgb[2 * d:], dxd.double().sum(0)))
    assert torch.equal((dxd == 0).cpu(), ~kb_out | (dx == 0).cpu()) and int((dx == 0).sum()) == 0
    assert e["dx"] < tol(dt) and e["dxd"] < tol(dt) and e["dgamma"] < 1e-4 and e["dbeta"] < 1e-4 and e["colsum"] < 1e-4, e
    print(f"layernorm dropout {dt} {M}x{d}: {e}")


@pytest.mark.parametrize("M,K,family", [(8192, 256, "gemm_wsr_lnb"), (9000, 256, "gemm_wsr_lnb"), (24577, 1024, "nt_lnb"), (30000, 512, "nt_lnb")])
def test_fused_layernorm_backward_dropout_matches_fp64_with_restated_masks(M, K, family):
    """dy = A W^T + residual, the backward of the LayerNorm whose output y was kept, then dx_drop = dx * keep / (1 - p) with the restated
    mask of the dense layer in front; the third block of dgb = column sums of the stored dx_drop.  Setup and bounds of
    test_layernorm_backward_in_the_data_gradient_epilogue (fp64 autograd: dx 3e-2, column sums 1e-4)."""
    _lib, L = _setup()
    H = _lib.hip()
    N, p, site = 256, 0.1, du.site_id(0, du.SITE_AO)
    g = torch.Generator().manual_seed(M)
    A = torch.randn(M, K, generator=g).cuda().bfloat16()
    W = (torch.randn(N, K, generator=g) / math.sqrt(K)).cuda().bfloat16()
    R = torch.randn(M, N, generator=g).cuda().bfloat16()
    x = (torch.randn(M, N, generator=g) * 1.5 + 0.3).cuda()
    gam = (1 + 0.1 * torch.randn(N, generator=g)).cuda()
    bet = (0.1 * torch.randn(N, generator=g)).cuda()
    xd = x.double().requires_grad_(True)
    gd, bd = gam.double().requires_grad_(True), bet.double().requires_grad_(True)
    yref = torch.nn.functional.layer_norm(xd, (N,), gd, bd, 1e-12)
    y = yref.detach().float().bfloat16()
    stats = torch.stack([x.double().mean(1), 1.0 / torch.sqrt(x.double().var(1, unbiased=False) + 1e-12)], 1).float().contiguous()
    rng = rng_t()
    dx = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
    dxd = torch.full((M, N), float("nan"), device="cuda", dtype=torch.bfloat16)
    tmp = torch.empty(M, N, device="cuda", dtype=torch.bfloat16)
    part = torch.empty(max(256, (M + 63) // 64) * 3 * N, device="cuda")
    dgb = torch.full((3 * N,), float("nan"), device="cuda")
    H.pmgt_launch_trace_reset()
    _lib.check(L.pmgt_op_linear_ln_bwd(P(A), K, P(W), K, M, N, K, P(R), N, P(y), P(stats), P(gam), P(bet), P(tmp), P(dx), P(dxd),
                                       p, site, P(rng), P(part), P(dgb), stream()))
    torch.cuda.synchronize()
    assert H.pmgt_launch_trace_count(family.encode()) == 1
    yref.backward(A.double() @ W.double().T + R.double())
    km, kb = keep_t(site, M, N, p, "cuda")
    e = dict(dx=rel_err(dx, xd.grad), dxd=rel_err(dxd, xd.grad * km), colsum=rel_err(dgb[2 * N:], dxd.double().sum(0)),
             dgamma=rel_err(dgb[:N], gd.grad), dbeta=rel_err(dgb[N:2 * N], bd.grad))
    zero_dx = int((dx == 0).sum())
    assert zero_dx == 0 and torch.equal(dxd == 0, ~kb)
    assert e["dx"] < 3e-2 and e["dxd"] < 3e-2 and e["colsum"] < 1e-4 and e["dgamma"] < 1.5e-2 and e["dbeta"] < (1e-3 if K == 256 else 5e-3), e
    print(f"fused layernorm backward dropout {family} M={M} K={K}: {e}")


# ------------------------------------------------------------------------------------------- attention
def attn_ref(qkvc, mask, H, beta, m1=None, m2=None):
    """_attn_ref of test_ops_gpu.py with optional multipliers m1 / m2 [T, H, S, S] (keep / (1 - p)) on each softmax branch BEFORE the
    beta mix (pmgt/pmgt/modeling_pmgt.py:457-458,509-513,519-521)."""
    T, S, d4 = qkvc.shape
    d = d4 // 4
    dh = d // H

    def heads(x):
        return x.view(T, S, H, dh).permute(0, 2, 1, 3)

    q, k, v, c = (heads(qkvc[..., i * d:(i + 1) * d]) for i in range(4))
    add = (1.0 - mask)[:, None, None, :] * -10000.0
    rho = torch.linalg.norm(c, dim=-1, keepdim=True)
    s1 = 1.0 - (c @ c.transpose(-1, -2)) / (rho @ rho.transpose(-1, -2)) + torch.eye(S, dtype=qkvc.dtype) + add
    s2 = (q @ k.transpose(-1, -2)) / math.sqrt(dh) + add
    a1, a2 = torch.softmax(s1, -1), torch.softmax(s2, -1)
    if m1 is not None:
        a1, a2 = a1 * m1, a2 * m2
    w = beta * a1 + (1 - beta) * a2
    return (w @ v).permute(0, 2, 1, 3).reshape(T, S, d), w


def attn_masks(T, H, S, p, s1, s2):
    """row (t * H + h) * S + i, column j"""
    m1, k1 = keep_t(s1, T * H * S, S, p)
    m2, k2 = keep_t(s2, T * H * S, S, p)
    sh = (T, H, S, S)
    return m1.reshape(sh), m2.reshape(sh), k1.reshape(sh), k2.reshape(sh)


def ragged_mask(T, S, stride=5):
    mask = torch.ones(T, S)
    for t in range(T):            # ragged valid lengths, position 0 always valid
        mask[t, 1 + (t * stride) % S:] = 0
    mask[0] = 1
    return mask


def expected_zero_probs(mask, beta, k1, k2):
    """w == 0 exactly where the key is masked (exp(-10000) underflows; not a mask decision: known from the key mask) or every live
    branch is dropped."""
    dead = torch.ones_like(k1)
    if beta != 0.0:
        dead &= ~k1
    if beta != 1.0:
        dead &= ~k2
    return dead | (mask == 0)[:, None, None, :]


ATTN_CASES = [
    # dt, path options, T, S, H, dh, beta
    ("fp32", (), 5, 16, 4, 16, 0.5), ("fp32", (), 3, 6, 2, 64, 0.3), ("fp32", (), 9, 33, 2, 32, 0.5), ("fp32", (), 3, 17, 2, 64, 0.3),
    ("fp32", (), 4, 32, 1, 128, 1.0),
    ("bf16", ("valu_attention",), 5, 16, 4, 16, 0.5), ("bf16", ("valu_attention",), 9, 33, 2, 32, 0.3), ("bf16", ("valu_attention",), 3, 17, 2, 64, 1.0),
    ("bf16", ("valu_attention",), 3, 6, 2, 64, 0.5),
    ("bf16", (), 7, 32, 8, 32, 0.5), ("bf16", (), 5, 48, 3, 64, 0.3), ("bf16", (), 11, 64, 8, 32, 1.0),                  # attn_fwd_mfma + cooperative backward
    ("bf16", ("wave_attention_bwd",), 7, 32, 8, 32, 0.5), ("bf16", ("wave_attention_bwd",), 5, 48, 3, 64, 0.3),          # attn_bwd_mfma: one wave per (sequence, head)
    ("bf16", ("wave_attention_bwd",), 4, 32, 1, 128, 1.0),
    ("bf16", (), 7, 64, 3, 64, 0.3), ("bf16", ("no_tile_attention",), 7, 64, 3, 64, 0.3),                                # S = 64 / dh = 64: tile and cooperative forms
    ("bf16", (), 9, 64, 8, 64, 0.5),
]


@pytest.mark.parametrize("dt,opts,T,S,H,dh,beta", ATTN_CASES)
def test_attention_dropout_matches_fp64_autograd_with_restated_masks(dt, opts, T, S, H, dh, beta):
    """Context, reported probabilities and dQ | dK | dV | dC of every attention implementation behind pmgt_op_attention_fwd / _bwd with
    dropout 0.2 on both branches, against fp64 autograd through the restated-mask reference: ragged key masks, S not a multiple of 4 on
    the generic kernel, beta in {0.3, 0.5, 1}.  Bounds of test_attention_fwd_bwd (probabilities 1e-5 / 2e-2, context tol(dt), gradient
    2e-4 / 3e-2; the S = 64 tile forms per block at 3e-2 as test_attention_tile_forms_match_the_oracle_restatement)."""
    _lib, L = _setup()
    Hh = _lib.hip()
    code, tdt = DT[dt]
    d, p, s1, s2 = H * dh, 0.2, du.site_id(1, du.SITE_A1), du.site_id(1, du.SITE_A2)
    g = torch.Generator().manual_seed(S * 100 + dh + H)
    x = torch.randn(T, S, 4 * d, generator=g) * (0.7 if S == 64 and dh == 64 else 1.0)
    dctx = torch.randn(T, S, d, generator=g)
    mask = ragged_mask(T, S, 13 if S == 64 else 5)
    xd, md, dod = to_dev(x, tdt), mask.cuda(), to_dev(dctx, tdt)
    rng = rng_t()
    m1, m2, k1, k2 = attn_masks(T, H, S, p, s1, s2)
    xr = rounded(x, tdt).requires_grad_(True)
    ref, w = attn_ref(xr, mask.double(), H, beta, m1, m2)
    ref.backward(rounded(dctx, tdt))
    L.use(*opts)
    try:
        ctx = torch.full((T, S, d), float("nan"), device="cuda", dtype=tdt)
        probs = torch.full((T, H, S, S), float("nan"), device="cuda")
        dx = torch.full((T, S, 4 * d), float("nan"), device="cuda", dtype=tdt)
        Hh.pmgt_launch_trace_reset()
        _lib.check(L.pmgt_op_attention_fwd(code, P(xd), P(md), P(ctx), P(probs), T, S, H, dh, beta, p, s1, s2, P(rng), stream()))
        _lib.check(L.pmgt_op_attention_bwd(code, P(xd), P(md), P(dod), P(dx), T, S, H, dh, beta, p, s1, s2, P(rng), stream()))
        torch.cuda.synchronize()
        tiles = (int(Hh.pmgt_launch_trace_count(b"attn_tiles_fwd")), int(Hh.pmgt_launch_trace_count(b"attn_tiles_bwd")))
    finally:
        L.use()
    assert tiles == ((1, 1) if (dt == "bf16" and S == 64 and dh == 64 and not opts) else (0, 0)), tiles
    want0 = expected_zero_probs(mask, beta, k1, k2)
    got0 = (probs == 0).cpu()
    assert torch.equal(got0, want0), (int((got0 != want0).sum()), "of", got0.numel())
    e = dict(probs=rel_err(probs, w.detach()), ctx=rel_err(ctx, ref.detach()))
    assert e["probs"] < (1e-5 if dt == "fp32" else 2e-2) and e["ctx"] < tol(dt), e
    if S == 64 and dh == 64:
        for m in range(4):          # dQ, dK, dV, dC blocks separately (their scales differ)
            e[f"d{'QKVC'[m]}"] = rel_err(dx[..., m * d:(m + 1) * d], xr.grad[..., m * d:(m + 1) * d])
            assert e[f"d{'QKVC'[m]}"] < 3e-2 or (beta == 1.0 and m < 2), e
    else:
        e["dx"] = rel_err(dx, xr.grad)
        assert e["dx"] < (2e-4 if dt == "fp32" else 3e-2), e
    print(f"attention dropout {dt} {opts} T={T} S={S} H={H} dh={dh} beta={beta}: {e}")


def _fused_inputs(T, H, seed, full_masked=False):
    S, dh = 32, 32
    d = H * dh
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(T, S, d, generator=g)
    W = torch.randn(4 * d, d, generator=g) / math.sqrt(d)
    bias = torch.randn(4 * d, generator=g) * 0.1
    dctx = torch.randn(T, S, d, generator=g)
    mask = ragged_mask(T, S, 7)
    if full_masked:
        mask[1] = 0                      # a fully masked sequence: the -10000 cancels in both softmaxes
    return S, dh, d, x, W, bias, dctx, mask


@pytest.mark.parametrize("T,H,beta,flags,family", [(33, 8, 0.5, 0, "qkvc_attn_fwd"), (33, 8, 0.3, 1, "qkvc_attn_fwd"), (130, 4, 0.5, 1, "qkvc_attn_fwd"),
                                                   (33, 8, 1.0, 1, "qkvc_attn_fwd"), (33, 8, 1.0, 3, "qkvc_attn_fwd_vc"), (7, 4, 1.0, 2, "qkvc_attn_fwd_vc")])
def test_fused_qkvc_attention_forward_dropout_matches_fp64_with_restated_masks(T, H, beta, flags, family):
    """qkvc_attn_fwd (both column layouts) and its beta = 1 form: Q|K|V|C against x W^T + b (4e-3), the context against the fp64
    restated-mask reference evaluated on the Q|K|V|C the kernel stored (tol(bf16): the bounds of
    test_fused_qkvc_attention_matches_the_two_kernel_path at dropout 0).  Ragged masks and one fully masked sequence."""
    _lib, L = _setup()
    Hh = _lib.hip()
    S, dh, d, x, W, bias, _, mask = _fused_inputs(T, H, T * 10 + H, full_masked=True)
    p, s1, s2 = 0.1, du.site_id(3, du.SITE_A1), du.site_id(3, du.SITE_A2)
    xd, Wd, bd, md = to_dev(x, torch.bfloat16), to_dev(W, torch.bfloat16), bias.cuda(), mask.cuda()
    rng = rng_t()
    qk = torch.full((T, S, 4 * d), float("nan"), device="cuda", dtype=torch.bfloat16)
    cx = torch.full((T, S, d), float("nan"), device="cuda", dtype=torch.bfloat16)
    Hh.pmgt_launch_trace_reset()
    _lib.check(L.pmgt_op_qkvc_attention_fwd_ex(P(xd), P(Wd), P(bd), P(md), P(qk), P(cx), T, S, H, dh, beta, p, s1, s2, P(rng), flags, stream()))
    torch.cuda.synchronize()
    assert Hh.pmgt_launch_trace_count(family.encode()) == 1 and Hh.pmgt_launch_trace_count(b"qkvc_attn_fwd") == 1
    q = (_from_head_major(qk, H, dh) if flags & 1 else qk).float().cpu().double()
    lo = 2 * d if flags & 2 else 0
    if flags & 2:
        assert torch.isnan(q[..., :lo]).all()        # the vc form neither projects nor stores Q | K
        q[..., :lo] = 0.0
    qr = rounded(x, torch.bfloat16).reshape(T * S, d) @ rounded(W, torch.bfloat16).T + bias.double()
    m1, m2, _, _ = attn_masks(T, H, S, p, s1, s2)
    ref, _ = attn_ref(q, mask.double(), H, beta, m1, m2)
    e = dict(qkvc=rel_err(q.reshape(T * S, 4 * d)[:, lo:], qr[:, lo:]), ctx=rel_err(cx, ref))
    assert torch.isfinite(cx.float()).all() and e["qkvc"] < 4e-3 and e["ctx"] < tol("bf16"), e
    for t in range(T):
        assert rel_err(cx[t], ref[t]) < tol("bf16"), t
    print(f"fused qkvc forward dropout {family} T={T} H={H} beta={beta} flags={flags}: {e}")


@pytest.mark.parametrize("T,H,beta,flags,family", [(23, 8, 0.5, 1, "attn_bwd_wgrad"), (7, 8, 0.3, 0, "attn_bwd_wgrad"), (700, 8, 0.5, 1, "attn_bwd_wgrad"),
                                                   (2, 4, 0.5, 0, "attn_bwd_wgrad"), (33, 8, 1.0, 3, "attn_bwd_wgrad_vc"), (9, 4, 1.0, 2, "attn_bwd_wgrad_vc"),
                                                   (33, 8, 1.0, 7, "attn_bwd_wgrad_vc2"), (700, 8, 1.0, 7, "attn_bwd_wgrad_vc2")])
def test_fused_attention_backward_dropout_matches_fp64_autograd_with_restated_masks(T, H, beta, flags, family):
    """attn_bwd_wgrad (both layouts, odd sequence counts, T = 700: more steps than one per workgroup) and the beta = 1 forms (one and
    two heads per step): dQ | dK | dV | dC against fp64 autograd through the restated-mask reference at the dropout-off bound of
    test_attention_backward_fused_with_qkvc_weight_gradient (2e-2); dW / db partials against the sums of what the kernel stored (1e-4)."""
    _lib, L = _setup()
    Hh = _lib.hip()
    S, dh, d, xin, _, _, dctx, mask = _fused_inputs(T, H, T * 10 + H + 1)
    g = torch.Generator().manual_seed(T + H)
    qkvc = torch.randn(T, S, 4 * d, generator=g)
    p, s1, s2 = 0.2, du.site_id(0, du.SITE_A1), du.site_id(0, du.SITE_A2)
    qd, dod, xd, md = to_dev(qkvc, torch.bfloat16), to_dev(dctx, torch.bfloat16), to_dev(xin, torch.bfloat16), mask.cuda()
    hm, vc, vc2 = flags & 1, bool(flags & 2), bool(flags & 4)
    q_in = _to_head_major(qd, H, dh) if hm else qd
    parts = Hh.pmgt_op_attention_bwd_wgrad_vc2_parts(H) if vc2 else L.pmgt_op_attention_bwd_wgrad_parts(H)
    rows = 2 * d if vc2 else 4 * d
    rng = rng_t()
    dx = torch.full((T, S, 4 * d), float("nan"), device="cuda", dtype=torch.bfloat16)
    slab = torch.full((parts, rows, d), float("nan"), device="cuda")
    bslab = torch.full((parts, rows), float("nan"), device="cuda")
    Hh.pmgt_launch_trace_reset()
    _lib.check(L.pmgt_op_attention_bwd_wgrad(P(q_in), P(md), P(dod), P(xd), P(dx), P(slab), P(bslab), T, H, beta, p, s1, s2, P(rng), flags, stream()))
    torch.cuda.synchronize()
    assert Hh.pmgt_launch_trace_count(family.encode()) == 1 and Hh.pmgt_launch_trace_count(b"attn_bwd_wgrad") == 1
    got = (_from_head_major(dx, H, dh) if hm else dx).float().cpu().double()
    lo = 2 * d if vc else 0
    if vc:
        assert torch.isnan(got[..., :lo]).all()          # dQ / dK are not written at beta = 1
    assert torch.isfinite(got[..., lo:]).all() and torch.isfinite(slab).all() and torch.isfinite(bslab).all()
    m1, m2, _, _ = attn_masks(T, H, S, p, s1, s2)
    xr = rounded(qkvc, torch.bfloat16).requires_grad_(True)
    ref, _ = attn_ref(xr, mask.double(), H, beta, m1, m2)
    ref.backward(rounded(dctx, torch.bfloat16))
    e = dict(dx=rel_err(got[..., lo:], xr.grad[..., lo:]))
    assert e["dx"] < 2e-2, e
    G = got[..., lo:].reshape(T * S, 4 * d - lo)
    X = xd.double().reshape(T * S, d).cpu()
    dW, db = slab.double().sum(0).cpu(), bslab.double().sum(0).cpu()
    if vc and not vc2:
        assert float(dW[:lo].abs().max()) == 0.0 and float(db[:lo].abs().max()) == 0.0
        dW, db = dW[lo:], db[lo:]
    e["dW"] = rel_err(dW, G.T @ X)
    e["db"] = float((db - G.sum(0)).abs().max()) / float(G.abs().sum(0).max())
    assert e["dW"] < 1e-4 and e["db"] < 1e-4, e
    print(f"fused attention backward dropout {family} T={T} H={H} beta={beta} flags={flags}: {e}")


# ------------------------------------------------------------------------------------------- embedding
@pytest.mark.parametrize("dt,phase,nf,d,S,Tq,store_pre,tok8", [("fp32", 0, 3, 384, 31, 6, True, (0, 0)), ("bf16", 0, 2, 256, 32, 7, True, (0, 0)),
                                                               ("fp32", 2, 2, 384, 31, 5, True, (0, 0)), ("bf16", 2, 3, 512, 32, 4, True, (0, 0)),
                                                               ("bf16", 2, 2, 256, 31, 9, False, (1, 2)), ("bf16", 2, 2, 256, 32, 12, True, (1, 1))])
def test_embedding_dropout_mask_is_the_restated_one(dt, phase, nf, d, S, Tq, store_pre, tok8):
    """h0 = dropout(LN(x)) and dF from dropout(dh0): phase 0, phase 2 and the embed_tok8 form (bf16, d = 256, odd S).  The harness of
    test_rowops_gpu.py builds its fp64 reference from the zero pattern of the device's h0; here that pattern must EQUAL the restated
    mask (row = token row m, column = channel; LayerNorm outputs of random rows are never exactly zero: nothing is left out), so its
    value checks (`_check_embed`, the dropout-off bounds) are checks against the restated mask."""
    from tests import test_rowops_gpu as tr
    p, M = 0.1, S * Tq
    res = tr._run_embed(dt, phase, nf, d, M, S, 60, drop_p=p, store_pre=store_pre, seed=5)
    assert res["tok8"] == tok8, res["tok8"]
    want = du.keep(4321, 9, 3, M, d, p)                  # _run_embed: rng = {4321, 9}, site 3
    got = (res["keep"] != 0).numpy()
    assert np.array_equal(got, want), int((got != want).sum())
    assert abs(float(res["keep"].max()) - 1.0 / (1.0 - p)) < 1e-12
    tr._check_embed(res, phase, nf, d, M)
