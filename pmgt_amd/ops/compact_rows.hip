// Single-kernel entry points (include/pmgt_ops.h) of the compacted-row forms of the last-layer shortcut: the launch is sized for a capacity on the
// host, the live row count is read on the device (m_dev), A / the residual / Q may come through a row list.  Host code only; every kernel
// launched here is the engine's, through the host function the engine calls.  (Kept out of csrc/: bench.py fingerprints the kernel sources
// there, and these entries launch nothing of their own.)
#include "../../include/pmgt_ops.h"
#include "../csrc/gemm.h"
#include "../csrc/rowops.h"

using namespace pmgt;

namespace {

void* g_zero_page = nullptr;      // >= 16 B of device zeros: the padding source of the LDS-DMA weight-gradient kernels (GemmTN::zeros)
const void* zero_page() {
    if (!g_zero_page) {
        if (hipMalloc(&g_zero_page, 4096) != hipSuccess || hipMemset(g_zero_page, 0, 4096) != hipSuccess) g_zero_page = nullptr;
    }
    return g_zero_page;
}

#define RUN(x)                                                                                    \
    do {                                                                                          \
        int rc__ = (x);                                                                           \
        if (rc__ != 0) return rc__;                                                               \
    } while (0)

// The dispatcher of one linear layer, restated from linear<T>() of csrc/engine.hip (which is local to that file) branch for branch, less the
// phase timers: full-row tile at N = 512, the 256 x 256 tile with the LayerNorm epilogue at N = 256 / K > 512, the weight-stationary
// streaming kernels (which pick the role-split forms themselves), else the tiled kernel; LayerNorm as its own launch -- with the same
// device-side row count -- wherever it is not fused.
template <typename T>
int linear_rows(const GemmWS& g, hipStream_t st) {
    if constexpr (sizeof(T) == 2) {
        if (g.ln_out && gemm_rowln_ok(g)) return gemm_rowln(g, st);
        if (g.ln_out && gemm_nt_lnf_ok(g)) return gemm_nt_lnf(g, st);
        if (!(g.opts & OPT_TILE_GEMM) && gemm_ws_supported(g)) {
            PMGT_CHECK(!g.skip_c || gemm_ws_fuses_ln(g), -2, "linear: skip_c needs the fused-LayerNorm form");
            RUN(gemm_ws(g, st));
            if (g.ln_out && !gemm_ws_fuses_ln(g))
                RUN(ln_fwd<T>((const T*)g.C, (T*)g.ln_out, g.ln_stats, g.ln_gamma, g.ln_beta, g.M, g.N, g.ln_eps, DropCfg{nullptr, 0.f, 0}, st,
                              g.m_dev, g.q8, g.q8_scale));
            return 0;
        }
    }
    PMGT_CHECK(!g.skip_c, -2, "linear: skip_c needs the fused-LayerNorm form");
    RUN(gemm_nt<T>(g, st));
    if (g.ln_out)
        RUN(ln_fwd<T>((const T*)g.C, (T*)g.ln_out, g.ln_stats, g.ln_gamma, g.ln_beta, g.M, g.N, g.ln_eps, DropCfg{nullptr, 0.f, 0}, st, g.m_dev,
                      g.q8, g.q8_scale));
    return 0;
}

}  // namespace

extern "C" {

// pmgt_op_linear in the form the engine launches for the tail of the shortcut layer: A rows through a_rows, the residual through the same
// list (res_gather), live rows = min(M, *m_dev).  skip_c stays false, as ln_from_y_applies() decides for compacted rows.
int pmgt_op_linear_rows(int dtype, const void* A, int64_t lda, const int64_t* a_rows, const void* B, int64_t ldb, void* C, int64_t ldc, int M,
                        int N, int K, const float* bias, int epilogue, void* aux, int64_t ldaux, const void* residual, int64_t ldr,
                        int res_gather, float drop_p, uint32_t drop_site, const uint64_t* rng, void* ln_out, float* ln_stats,
                        const float* ln_gamma, const float* ln_beta, float ln_eps, const int* m_dev, uint32_t path_opts, void* stream) {
    PMGT_CHECK(A && B && C, -2, "pmgt_op_linear_rows: NULL operand (A, B and C are required)");
    PMGT_CHECK(epilogue == 0 || aux, -2, "pmgt_op_linear_rows: epilogue %d needs aux", epilogue);
    PMGT_CHECK(!res_gather || (a_rows && residual), -2, "pmgt_op_linear_rows: res_gather needs a_rows and a residual");
    PMGT_CHECK(!ln_out || (ln_stats && ln_gamma && ln_beta), -2, "pmgt_op_linear_rows: ln_out needs ln_stats, ln_gamma and ln_beta");
    GemmWS g; g.opts = path_opts;
    g.A = A; g.lda = lda; g.a_rows = a_rows; g.B = B; g.ldb = ldb; g.C = C; g.ldc = ldc; g.M = M; g.N = N; g.K = K;
    g.bias = bias; g.epi = epilogue; g.aux = aux; g.ldaux = ldaux; g.res = residual; g.ldr = ldr; g.res_gather = res_gather != 0;
    g.drop = DropCfg{rng, rng ? drop_p : 0.f, drop_site}; g.m_dev = m_dev;
    g.ln_out = ln_out; g.ln_stats = ln_stats; g.ln_gamma = ln_gamma; g.ln_beta = ln_beta; g.ln_eps = ln_eps;
    if (dtype == PMGT_DTYPE_BF16) return linear_rows<bf16>(g, (hipStream_t)stream);
    return linear_rows<float>(g, (hipStream_t)stream);
}

// the LayerNorm backward of the compacted tail: x stored (beta_y = NULL), rows < min(M, *m_dev); the grid and `part` are sized for M
int pmgt_op_layernorm_bwd_rows(int dtype, const void* dy, const void* x, const float* stats, const float* gamma, void* dx, void* dx_drop,
                               float* part, float* dgamma_dbeta, int M, int d, float in_drop_p, uint32_t in_site, float out_drop_p,
                               uint32_t out_site, const uint64_t* rng, const int* m_dev, void* stream) {
    DropCfg di{rng, rng ? in_drop_p : 0.f, in_site}, dout{rng, rng ? out_drop_p : 0.f, out_site};
    hipStream_t st = (hipStream_t)stream;
    if (dtype == PMGT_DTYPE_BF16)
        RUN(ln_bwd<bf16>((const bf16*)dy, (const bf16*)x, stats, gamma, (bf16*)dx, (bf16*)dx_drop, part, M, d, di, dout, st, m_dev, nullptr));
    else
        RUN(ln_bwd<float>((const float*)dy, (const float*)x, stats, gamma, (float*)dx, (float*)dx_drop, part, M, d, di, dout, st, m_dev, nullptr));
    return slab_reduce(part, ln_bwd_parts(M), 3 * d, dgamma_dbeta, false, st);
}

// the weight + bias gradient of the compacted tail as the engine's wgrad helper launches it: device-side row count, optional gather on Q,
// and the splits from m_for_splits (the engine: max(256, capacity / 3)) instead of from M
int pmgt_op_gemm_tn_bias_rows(int dtype, const void* P, int64_t ldp, const void* Q, int64_t ldq, const int64_t* q_rows, int M, int m_for_splits,
                              int N1, int N2, float* slab, float* out, float* bias_slab, float* bias_out, int accumulate, const int* m_dev,
                              uint32_t path_opts, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    PMGT_CHECK(!bias_slab || bias_out, -2, "pmgt_op_gemm_tn_bias_rows: bias_slab needs bias_out");
    GemmTN g; g.opts = path_opts;
    g.P = P; g.ldp = ldp; g.Q = Q; g.ldq = ldq; g.q_rows = q_rows; g.M = M; g.N1 = N1; g.N2 = N2; g.slab = slab; g.bias_slab = bias_slab;
    g.m_dev = m_dev; g.zeros = zero_page();
    g.splits = gemm_tn_pick_splits(m_for_splits, N1, N2, dtype != PMGT_DTYPE_F32 ? 64 : 32, path_opts);
    PMGT_CHECK(g.splits <= 512, -2, "pmgt_op_gemm_tn_bias_rows: bias_slab holds at most 512 splits");
    RUN(dtype != PMGT_DTYPE_F32 ? gemm_tn<bf16>(g, st) : gemm_tn<float>(g, st));
    RUN(slab_reduce(slab, g.splits, (int64_t)N1 * N2, out, accumulate != 0, st));
    if (!bias_slab) return 0;
    return slab_reduce(bias_slab, g.splits, N1, bias_out, accumulate != 0, st);
}

}  // extern "C"
