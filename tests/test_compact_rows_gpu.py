"""The compacted-row kernels of the last-layer shortcut, one kernel at a time: the tail of the last encoder layer runs on the rows the loss
reads only (csrc/engine.hip at `sc`), the launch sized for the capacity M on the host and the live row count read on the device (m_dev).
Entries: pmgt_op_linear_rows (gather on A, gathered residual, m_dev through the engine's linear() dispatcher), pmgt_op_layernorm_bwd_rows and
pmgt_op_gemm_tn_bias_rows (q_rows, m_dev, accumulate, splits sized from m_for_splits = max(256, M / 3) as the engine sizes them).

Layout of every case: rows < count hold seeded data; rows >= count hold NaN in every input that is not gathered (A, residual, the GELU'
pre-activation, dy, x, stats, P, Q); the dead entries of a_rows / q_rows point at ONE all-NaN row of the table (never out of range); every
output has guard rows past M and is filled with a NaN of a payload no arithmetic produces (SENT), so "not written" is a bit comparison.
Each case asserts
  a. live rows against fp64 torch on the bf16- / fp32-rounded inputs, at the tolerance of the sibling test of the same kernel: tol(dt) of
     test_ops_gpu.py for GEMM and LayerNorm outputs, 1e-3 for {mean, rstd} (test_dropout_ops_gpu.py), 1e-4 for fp32-accumulated sums (column
     sums against the values the kernel itself stored), 1e-5 for the fp32 weight gradient (test_gemm_tn);
  b. reductions (dgamma, dbeta, the dx column sum, weight and bias gradient) finite and equal to the fp64 sums over the LIVE rows; count == 0:
     exact zeros, or exactly the prior contents when accumulating;
  c. rows [count, M) and the guard rows keep SENT in C, aux, ln_out, ln_stats, dx and dx_drop -- no kernel here writes a dead row;
  d. the launch trace shows the family the case is for (nt_tile, gemm_ws, gemm_wsr, gemm_wsr512, gemm_rowln, tn_dma, tn_dma_gather, tn_tile);
and, where the dense call (m_dev = NULL, all M rows live, inputs gathered beforehand) runs the same family, that the live rows are BIT-EQUAL to
it (rows are independent, the K loop is the same).  For the gathered attention output in bf16 the pre-gathered dense call is a different family
(gemm_ws: the streaming kernel has no gather), so there the dense call keeps a_rows.

Counts per case: 0, 1, tile - 1, tile, tile + 1, a mid value that is no multiple of 8, M - 1, M for the kernel's row tile (WsCfg::TR = 32 / 64,
WsrCfg::TR = Wsr5Cfg::TR = 32, RL_BM = 128, the 128-row tile, ln_bwd_rows = 64, the 64-row chunk granule of the TN kernels).

The last test is the engine-level one: a shortcut step with FEW live rows in a workspace whose dead rows hold a previous step's values (many
live rows) must equal, bit for bit, the same step in a NaN-filled workspace."""
import pytest
import torch

from tests import dropout_util as du
from tests import golden_util as gu
from tests.test_dropout_ops_gpu import keep_t, rng_t
from tests.test_engine_gpu import dev_batch, make_engine
from tests.test_ops_gpu import DT, P, _setup, rel_err, stream, to_dev, tol

pytestmark = pytest.mark.gpu

GUARD = 3
# quiet NaNs with a payload: an operation on the canonical NaN of the poisoned inputs returns the canonical NaN, never these bits
SENT = {torch.bfloat16: (torch.int16, 0x7FE5), torch.float32: (torch.int32, 0x7FE5A5A5)}
FAMILIES = ("nt_tile", "nt_big", "nt_big_128", "nt_lnf", "gemm_ws", "gemm_wsr", "gemm_wsr512", "gemm_rowln", "tn_tile", "tn_dma", "tn_dma_gather",
            "tn_big", "tn_big_gather")


def sentinel(rows, cols, tdt):
    """[rows + GUARD, cols] of SENT."""
    it, bits = SENT[tdt]
    return torch.full((rows + GUARD, cols), bits, dtype=it, device="cuda").view(tdt)


def sentinel_flat(n, tdt=torch.float32):
    """[n + 64] of SENT."""
    it, bits = SENT[tdt]
    return torch.full((n + 64,), bits, dtype=it, device="cuda").view(tdt)


def untouched(t):
    it, bits = SENT[t.dtype]
    return bool((t.contiguous().view(it) == bits).all())


def poisoned(x, count):
    y = x.clone()
    y[count:] = float("nan")
    return y


def cnt_t(count):
    return torch.tensor([count], dtype=torch.int32, device="cuda")


def counts_for(tiles, M):
    mid = (M // 2) | 3                  # ...11 in binary: no multiple of 8
    c = {0, 1, mid, M - 1, M}
    for t in tiles:
        c |= {t - 1, t, t + 1}
    return sorted(x for x in c if 0 <= x <= M)


def trace(H):
    return {f: n for f in FAMILIES for n in [int(H.pmgt_launch_trace_count(f.encode()))] if n}


def gelu_grad(x):
    x = x.double().clone().requires_grad_(True)
    torch.nn.functional.gelu(x).sum().backward()
    return x.grad


# ------------------------------------------------------------------------------------------- linear (forward GEMMs and data gradients)
def _linear_case(dt, M, N, K, epi, res, drop, ln, gather, family, tiles, opts=()):
    """Runs one compacted linear at every count of counts_for(tiles, M); returns the largest live-row errors."""
    _lib, L = _setup()
    H = _lib.hip()
    code, tdt = DT[dt]
    site = du.site_id(1, du.SITE_AO)
    g = torch.Generator().manual_seed(M * 3 + N + K + epi)
    R = M + 57                                          # table rows of the gathered forms; row R - 1 is the all-NaN one
    A = to_dev(torch.randn(R if gather else M, K, generator=g), tdt)
    W = to_dev(torch.randn(N, K, generator=g) * 0.2, tdt)
    bias = torch.randn(N, generator=g).cuda()
    Rs = to_dev(torch.randn(R if gather else M, N, generator=g), tdt) if res else None
    aux_in = to_dev(torch.randn(M, N, generator=g), tdt) if epi == 2 else None
    gam = (1 + 0.1 * torch.randn(N, generator=g)).cuda()
    bet = (0.1 * torch.randn(N, generator=g)).cuda()
    rows = torch.randint(0, R - 1, (M,), generator=g).cuda() if gather else None
    if gather:
        A[R - 1] = float("nan")
        if res:
            Rs[R - 1] = float("nan")
    rng = rng_t() if drop > 0 else None
    Ag = A[rows] if gather else A
    Rg = (Rs[rows] if gather else Rs) if res else None

    # ---- fp64 reference of all M rows (rows are independent: row m of a call with count > m is row m of this)
    pre = Ag.double() @ W.double().T + bias.double()
    ref = {}
    if epi == 1:
        ref["aux"] = pre
        cref = torch.nn.functional.gelu(pre.to(tdt).double())
    elif epi == 2:
        cref = pre * gelu_grad(aux_in)
    else:
        cref = pre
    if drop > 0:
        cref = cref * keep_t(site, M, N, drop, "cuda")[0]
    if res:
        cref = cref + Rg.double()
    ref["C"] = cref
    if ln:
        x = cref.to(tdt).double()              # gemm.h: ln_out = LN(C) with C the storage-rounded epilogue result
        ref["ln"] = torch.nn.functional.layer_norm(x, (N,), gam.double(), bet.double(), 1e-12)
        ref["stats"] = torch.stack([x.mean(1), 1.0 / torch.sqrt(x.var(1, unbiased=False) + 1e-12)], 1)
    bound = {"C": tol(dt), "aux": tol(dt), "ln": tol(dt), "stats": 1e-3}

    def call(count, a, a_rows, r, r_gather, aux_src):
        out = {"C": sentinel(M, N, tdt)}
        if epi == 1:
            out["aux"] = sentinel(M, N, tdt)
        if ln:
            out["ln"], out["stats"] = sentinel(M, N, tdt), sentinel(M, 2, torch.float32)
        aux = out["aux"] if epi == 1 else aux_src
        cnt = None if count is None else cnt_t(count)
        L.use(*opts)
        H.pmgt_launch_trace_reset()
        _lib.check(L.pmgt_op_linear_rows(code, P(a), K, P(a_rows), P(W), K, P(out["C"]), N, M, N, K, P(bias), epi, P(aux), N, P(r), N,
                                         1 if r_gather else 0, drop, site, P(rng), P(out.get("ln")), P(out.get("stats")),
                                         P(gam) if ln else None, P(bet) if ln else None, 1e-12, P(cnt), stream()))
        torch.cuda.synchronize()
        L.use()
        return out, trace(H)

    # ---- dense calls: every row live, no device count
    dense = []
    d_out, d_tr = call(None, Ag, None, Rg, False, aux_in)              # inputs gathered beforehand
    dense.append((d_out, d_tr))
    if gather:
        dense.append(call(None, A, rows, Rs, res, aux_in))              # the gather kept
    same = [o for o, tr in dense if tr == {family: 1}]
    assert same, (family, [tr for _, tr in dense])
    for o in same:
        assert all(untouched(v[M:]) for v in o.values())

    worst = {k: 0.0 for k in ref}
    for count in counts_for(tiles, M):
        if gather:
            a, ar = A, rows.clone()
            ar[count:] = R - 1
            r = Rs
        else:
            a, ar, r = poisoned(A, count), None, (poisoned(Rs, count) if res else None)
        out, tr = call(count, a, ar, r, gather and res, poisoned(aux_in, count) if epi == 2 else None)
        assert tr == {family: 1}, (count, tr)          # (the host does not know the count: it launches for the capacity)
        for k, v in out.items():
            assert untouched(v[count:]), (k, count, "rows >= count (dead rows and guard rows) must keep the sentinel")
            if count == 0:
                continue
            live = v[:count]
            assert torch.isfinite(live.float()).all(), (k, count)
            e = rel_err(live, ref[k][:count])
            worst[k] = max(worst[k], e)
            print(f"compact linear {family} {dt} M={M} N={N} K={K} epi={epi} drop={drop} count={count} {k}: {e:.3g} (bound {bound[k]:g})")
            assert e < bound[k], (k, count, e)
            for o in same:
                assert torch.equal(live, o[k][:count]), (k, count, "live rows differ from the dense call of the same family")
    return worst


@pytest.mark.parametrize("dt,d,drop", [("bf16", 256, 0.0), ("bf16", 256, 0.1), ("bf16", 128, 0.0), ("bf16", 128, 0.1), ("fp32", 256, 0.1), ("fp32", 128, 0.0)])
def test_attention_output_on_gathered_rows(dt, d, drop):
    """BertSelfOutput of the shortcut layer as the engine launches it: A = ctx rows through need_rows, the residual = hin rows through the same
    list, bias, dropout, then LayerNorm.  A gather keeps the streaming kernels out (gemm_ws_supported), so this is the 128 x 128 tile + the
    standalone LayerNorm launch, both with m_dev.  Bit-equal to the dense call that keeps the gather (bf16) / to both dense calls (fp32)."""
    _linear_case(dt, 300, d, d, 0, True, drop, True, True, "nt_tile", (128,))


@pytest.mark.parametrize("N", [512, 1024])
def test_ffn1_gelu_with_stored_preactivation(N):
    """BertIntermediate on compacted rows: GELU, the pre-activation stored in aux (two 4-wave workgroups per CU, 32-row tiles)."""
    _linear_case("bf16", 200, N, 256, 1, False, 0.0, False, False, "gemm_ws", (32, 64))


@pytest.mark.parametrize("M,N,K,drop,family,tiles,opts", [
    (200, 256, 256, 0.0, "gemm_ws", (32, 64), ()),              # fused LayerNorm, 64-row tiles
    (200, 256, 256, 0.1, "gemm_ws", (32, 64), ()),
    (200, 256, 512, 0.1, "gemm_ws", (32, 64), ()),              # K = 512 form (one LDS buffer, LDS-DMA), fused LayerNorm
    (200, 256, 256, 0.1, "nt_tile", (128,), ("tile_gemm",)),    # tiled + the LayerNorm launch
    (8200, 256, 256, 0.1, "gemm_wsr", (32,), ()),               # role-split residual + LayerNorm
    (8200, 256, 256, 0.0, "gemm_wsr", (32,), ()),
    (8200, 256, 512, 0.1, "gemm_ws", (32, 64), ()),             # K = 512, N = 256 WITH LayerNorm stays on the lockstep kernel at any M (gemm_ws.hip: gemm_ws)
    (8200, 256, 512, 0.1, "gemm_wsr512", (32,), ("unfused_ln",)),      # ... the role-split K = 512 kernel + the LayerNorm launch
    (8200, 512, 512, 0.0, "gemm_wsr512", (32,), ("unfused_ln",)),
    (4100, 512, 512, 0.1, "gemm_rowln", (128,), ()),            # full-row tile, LayerNorm in the epilogue
    (4100, 512, 256, 0.0, "gemm_rowln", (128,), ()),
])
def test_ffn2_residual_layernorm(M, N, K, drop, family, tiles, opts):
    """BertOutput on compacted rows: bias, dropout, residual (compact order: no gather), LayerNorm -- every kernel the dispatcher has for it."""
    _linear_case("bf16", M, N, K, 0, True, drop, True, False, family, tiles, opts)


@pytest.mark.parametrize("M,N,K,epi,res,drop,family", [
    (200, 512, 256, 2, False, 0.0, "gemm_ws"),         # d ff_pre = (dY2 W2) gelu'(ff_pre)
    (200, 256, 512, 0, True, 0.0, "gemm_ws"),          # du = dff W1 + residual branch
    (200, 256, 256, 0, False, 0.0, "gemm_ws"),         # dctx = dYo Wo
    (8200, 512, 512, 0, False, 0.0, "gemm_wsr512"),    # the K = 512 role-split forms: plain (the epilogue role moves the A tiles) ...
    (8200, 512, 512, 1, False, 0.0, "gemm_wsr512"),    # ... GELU
    (8200, 512, 512, 2, False, 0.0, "gemm_wsr512"),    # ... GELU'
    (8200, 256, 512, 0, True, 0.1, "gemm_wsr512"),     # ... residual
])
def test_data_gradients_and_k512_role_split_epilogues(M, N, K, epi, res, drop, family):
    """The backward data gradients of the compacted tail (GELU', residual, plain) on the streaming kernel, and the four epilogues of the
    K = 512 role-split kernel from 8192 rows of capacity on."""
    _linear_case("bf16", M, N, K, epi, res, drop, False, False, family, (32, 64) if family == "gemm_ws" else (32,))


# ------------------------------------------------------------------------------------------- LayerNorm backward
@pytest.mark.parametrize("dt,d", [("bf16", 128), ("bf16", 256), ("bf16", 512), ("fp32", 256)])
@pytest.mark.parametrize("with_dxd,p", [(False, 0.0), (True, 0.0), (True, 0.1)])
def test_layernorm_backward_counts_live_rows_only(dt, d, with_dxd, p):
    """ln_bwd with m_dev, x stored (the compacted path keeps its LayerNorm inputs): dx / dx_drop of the live rows against fp64 autograd with
    the restated mask of the dense layer in front; dgamma, dbeta against the fp64 sums over the live rows, the third block against the column
    sums of the dx_drop (or dx) the kernel stored.  A workgroup past the live rows writes a zero partial (part is scratch: all of it is
    written); nothing else is."""
    _lib, L = _setup()
    code, tdt = DT[dt]
    M, site = 200, du.site_id(2, du.SITE_FO)
    g = torch.Generator().manual_seed(d + 7)
    x = to_dev(torch.randn(M, d, generator=g) * 2 + 0.5, tdt)
    dy = to_dev(torch.randn(M, d, generator=g), tdt)
    gam = (1 + 0.1 * torch.randn(d, generator=g)).cuda()
    xr = x.double().requires_grad_(True)
    gr = gam.double()
    mean, var = xr.detach().mean(1, keepdim=True), xr.detach().var(1, unbiased=False, keepdim=True)
    rstd = 1.0 / torch.sqrt(var + 1e-12)
    stats = torch.cat([mean, rstd], 1).float().contiguous()
    xh = (xr.detach() - mean) * rstd
    torch.nn.functional.layer_norm(xr, (d,), gr, None, 1e-12).backward(dy.double())
    dx_ref = xr.grad
    km = keep_t(site, M, d, p, "cuda")[0] if p > 0 else torch.ones(M, d, device="cuda", dtype=torch.float64)
    rng = rng_t() if p > 0 else None
    parts = (M + 63) // 64
    worst = {}
    for count in counts_for((64,), M):
        dx = sentinel(M, d, tdt)
        dxd = sentinel(M, d, tdt) if with_dxd else None
        part = sentinel(parts * 3, d, torch.float32)
        dgb = sentinel(3, d, torch.float32)
        dy_c, x_c, stats_c, cnt = poisoned(dy, count), poisoned(x, count), poisoned(stats, count), cnt_t(count)
        _lib.check(L.pmgt_op_layernorm_bwd_rows(code, P(dy_c), P(x_c), P(stats_c), P(gam), P(dx), P(dxd), P(part), P(dgb), M, d, 0.0, 0, p, site,
                                                P(rng), P(cnt), stream()))
        torch.cuda.synchronize()
        assert untouched(dx[count:]) and (dxd is None or untouched(dxd[count:])), count
        assert untouched(part[parts * 3:]) and untouched(dgb[3:]), count
        sums = dgb[:3]
        assert torch.isfinite(sums).all(), count
        if count == 0:
            assert bool((sums == 0).all())
            continue
        stored = (dxd if with_dxd else dx)[:count].double()
        e = dict(dx=rel_err(dx[:count], dx_ref[:count]),
                 dgamma=rel_err(sums[0], (dy.double() * xh)[:count].sum(0)), dbeta=rel_err(sums[1], dy.double()[:count].sum(0)),
                 colsum=rel_err(sums[2], stored.sum(0)))
        if with_dxd:
            e["dxd"] = rel_err(dxd[:count], (dx_ref * km)[:count])
        for k, v in e.items():
            worst[k] = max(worst.get(k, 0.0), v)
        print(f"compact ln_bwd {dt} d={d} dxd={with_dxd} p={p} count={count}: {e}")
        assert e["dx"] < tol(dt) and e.get("dxd", 0.0) < tol(dt) and e["dgamma"] < 1e-4 and e["dbeta"] < 1e-4 and e["colsum"] < 1e-4, (count, e)
    # the dense call (m_dev = NULL, every row live) is the same kernel: the live rows of a compacted call are bit-equal to it
    dx0 = sentinel(M, d, tdt)
    dxd0 = sentinel(M, d, tdt) if with_dxd else None
    part = sentinel(parts * 3, d, torch.float32)
    dgb = sentinel(3, d, torch.float32)
    _lib.check(L.pmgt_op_layernorm_bwd_rows(code, P(dy), P(x), P(stats), P(gam), P(dx0), P(dxd0), P(part), P(dgb), M, d, 0.0, 0, p, site, P(rng),
                                            None, stream()))
    count = 137
    dx = sentinel(M, d, tdt)
    dxd = sentinel(M, d, tdt) if with_dxd else None
    dy_c, x_c, stats_c, cnt = poisoned(dy, count), poisoned(x, count), poisoned(stats, count), cnt_t(count)
    _lib.check(L.pmgt_op_layernorm_bwd_rows(code, P(dy_c), P(x_c), P(stats_c), P(gam), P(dx), P(dxd), P(part), P(dgb), M, d, 0.0, 0, p, site,
                                            P(rng), P(cnt), stream()))
    torch.cuda.synchronize()
    assert torch.equal(dx[:count], dx0[:count]) and (not with_dxd or torch.equal(dxd[:count], dxd0[:count]))


# ------------------------------------------------------------------------------------------- weight + bias gradient
@pytest.mark.parametrize("dt,M,N1,N2,gather,family", [
    ("bf16", 3000, 256, 256, False, "tn_dma"),            # wgrad_ffn1 / ffn2 shape: P and Q in compact order, bias sums riding along
    ("bf16", 3000, 256, 256, True, "tn_dma_gather"),      # wgrad_attn_out: Q = ctx rows through need_rows
    ("bf16", 3001, 512, 256, False, "tn_dma"),            # ragged capacity, two N1 tiles
    ("bf16", 31744, 256, 256, False, "tn_dma"),           # steady state of the LDS-DMA ring
    ("bf16", 31744, 256, 1536, True, "tn_dma_gather"),
    ("fp32", 3000, 256, 64, False, "tn_tile"),
    ("fp32", 3000, 256, 64, True, "tn_tile"),
])
def test_weight_and_bias_gradient_sized_from_a_third_of_the_capacity(dt, M, N1, N2, gather, family):
    """wgrad of the compacted tail: splits from gemm_tn_pick_splits(max(256, M / 3)), row chunks re-derived on the device from the live count
    (which may lie below OR above the row count the splits were sized for).  Weight gradient = P[:count]^T Q[rows[:count]], bias gradient
    (no-gather forms, as in the engine) = column sums of P[:count]; overwrite into a sentinel-filled output and accumulate onto 1.5."""
    _lib, L = _setup()
    H = _lib.hip()
    code, tdt = DT[dt]
    g = torch.Generator().manual_seed(M + N1 + N2)
    mfs = max(256, M // 3)
    R = 4096
    Pm = to_dev(torch.randn(M, N1, generator=g) + 0.25, tdt)          # non-zero column means
    Q = to_dev(torch.randn(R if gather else M, N2, generator=g), tdt)
    rows = torch.randint(0, R - 1, (M,), generator=g).cuda() if gather else None
    if gather:
        Q[R - 1] = float("nan")
    with_bias = not gather
    nslab = int(L.pmgt_op_gemm_tn_slab_elems(code, mfs, N1, N2))
    tolr = 1e-5 if dt == "fp32" else 1e-4
    Pd, Qg = Pm.double(), (Q[rows] if gather else Q).double()
    worst = 0.0
    for count in sorted({0, 1, 63, 64, 65, (mfs - 37) | 1, (mfs + 101) | 1, M - 1, M}):
        p_in = poisoned(Pm, count)
        if gather:
            q_in, q_rows = Q, rows.clone()
            q_rows[count:] = R - 1
        else:
            q_in, q_rows = poisoned(Q, count), None
        ref = Pd[:count].T @ Qg[:count]
        bref = Pd[:count].sum(0)
        cnt = cnt_t(count)
        for acc in (0, 1):
            slab, bslab = sentinel_flat(nslab), sentinel_flat(512 * N1)
            out, bout = sentinel(N1, N2, torch.float32), sentinel_flat(N1)
            if acc:
                out[:N1] = 1.5
                bout[:N1] = 1.5
            H.pmgt_launch_trace_reset()
            _lib.check(L.pmgt_op_gemm_tn_bias_rows(code, P(p_in), N1, P(q_in), N2, P(q_rows), M, mfs, N1, N2, P(slab), P(out),
                                                   P(bslab) if with_bias else None, P(bout) if with_bias else None, acc, P(cnt), stream()))
            torch.cuda.synchronize()
            assert trace(H) == {family: 1}, (count, trace(H))
            assert untouched(out[N1:]) and untouched(bout[N1:]) and untouched(slab[nslab:]) and untouched(bslab[512 * N1:]), (count, acc)
            got = [(out[:N1], ref)] + ([(bout[:N1], bref)] if with_bias else [])
            for o, r in got:
                assert torch.isfinite(o).all(), (count, acc)
                if count == 0:
                    assert bool((o == (1.5 if acc else 0.0)).all()), (count, acc)
                elif acc:
                    assert float((o.double() - (r + 1.5)).abs().max()) <= tolr * max(float(r.abs().max()), 1.0) + 1e-6, (count, acc)
                else:
                    e = rel_err(o, r)
                    worst = max(worst, e)
                    assert e < tolr, (count, e)
    print(f"compact wgrad {family} {dt} M={M} N1={N1} N2={N2} m_for_splits={mfs}: worst {worst:.3g} (bound {tolr:g})")


# ------------------------------------------------------------------------------------------- the engine: stale dead rows
def test_stale_dead_rows_of_a_previous_step_do_not_reach_the_gradients():
    """bf16, dropout off, the shortcut on (want_hidden = False).  Engine A runs a step whose injection masks EVERY valid position (a large
    live count: the compacted buffers fill up), then -- gradients reset -- a step that masks one position per sequence: the rows between the
    two live counts still hold the first step's activations and gradients.  Engine B runs only the second step, in a workspace filled with
    NaN.  Loss and every gradient must be finite and bit-equal: no reduction of the compacted tail may see a row past the live count."""
    case = gu.model_case("m3")
    batch = dev_batch(case["batch"])
    ids = case["batch"][0]["node_ids"]
    valid = (ids != 0)
    valid[:, 0] = False

    def inject(mask):
        masked = torch.where(mask, torch.ones_like(ids), ids)
        full = torch.where(mask, ids, torch.full_like(ids, -1))
        return masked.cuda(), full.cuda()

    many = valid
    few = torch.zeros_like(valid)
    few[:, 1] = valid[:, 1]
    n_many, n_few = int(many.sum()), int(few.sum())
    assert 0 < n_few and 4 * n_few < n_many

    def second_step(eng):
        eng.grads.zero_()
        eng.rng_state[1] = 0
        out = eng.pretrain_step(batch, training=True, backward=True, nfr_inject=inject(few), want_hidden=False)
        torch.cuda.synchronize()
        assert int(out["nfr_count"].item()) == n_few
        return out["losses"].clone(), eng.grads.clone()

    a = make_engine(case, dtype="bf16")
    out = a.pretrain_step(batch, training=True, backward=True, nfr_inject=inject(many), want_hidden=False)
    assert int(out["nfr_count"].item()) == n_many
    loss_a, grads_a = second_step(a)

    b = make_engine(case, dtype="bf16")
    B, S = ids.shape
    n_seq = 2 * B + int(case["batch"][1]["node_ids"].shape[0])
    nbytes = int(b.lib.pmgt_workspace_bytes(b.h, n_seq, S, B, 1))
    b._ws = torch.full((nbytes // 4 + 1,), float("nan"), device="cuda").view(torch.uint8)      # what Engine._workspace hands to the step
    loss_b, grads_b = second_step(b)

    assert torch.isfinite(loss_a).all() and torch.isfinite(grads_a).all()
    assert torch.isfinite(loss_b).all() and torch.isfinite(grads_b).all()
    assert torch.equal(loss_a, loss_b)
    assert torch.equal(grads_a, grads_b), int((grads_a != grads_b).sum())
