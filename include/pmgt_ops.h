/*
 * pmgt_ops.h -- TEST AND A/B SURFACE of libpmgt_hip.so: single-kernel entry points (unit / parity tests of each kernel
 * against the oracle) and the catalogue of path options.  Not needed to use the engine (include/pmgt_capi.h is the
 * product ABI); same conventions as there.
 */
#ifndef PMGT_OPS_H
#define PMGT_OPS_H

#include "pmgt_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- path options ---------------------------------------------------------------------------------
 * Keys of the per-engine option setter declared in pmgt_capi.h, and the bit each one has in the `path_opts` argument of the pmgt_op_* entry
 * points below (which have no engine).  0 everywhere = the product path. */
#define PMGT_OPT_TILE_GEMM (1u << 0)                 /* "tile_gemm": register-staged 128 x 128 GEMM tiles only (no streaming kernel, LDS-DMA or 256 x 256 tiles) */
#define PMGT_OPT_VALU_ATTENTION (1u << 1)            /* "valu_attention": bf16 attention on the generic fp32-VALU kernel instead of the MFMA one */
#define PMGT_OPT_WAVE_ATTENTION_BWD (1u << 2)        /* "wave_attention_bwd": MFMA attention backward with one wave per (sequence, head) instead of cooperating waves */
#define PMGT_OPT_NO_SHORTCUT (1u << 3)               /* "no_shortcut": last layer on every token even when last_hidden is not requested */
#define PMGT_OPT_NO_FUSED_QKVC_ATTENTION (1u << 4)   /* "no_fused_qkvc_attention": projection GEMM and attention as two kernels */
#define PMGT_OPT_NO_HEAD_MAJOR (1u << 5)             /* "no_head_major": Q|K|V|C stays q | k | v | c between the fused forward and the backward */
#define PMGT_OPT_NO_TABLE_PROJECTION (1u << 6)       /* "no_table_projection": features projected per token even when the table is smaller than half the batch's tokens */
#define PMGT_OPT_NO_SEGMENT_SUM (1u << 7)            /* "no_segment_sum": table mode keeps the per-token weight-gradient GEMM of the feature projection */
#define PMGT_OPT_CONSUMER_QUANT (1u << 8)            /* "consumer_quant": fp8 mode, layer inputs quantised inside the fused forward instead of by their producer (bit-identical) */
#define PMGT_OPT_NO_FUSED_ATTENTION_BWD (1u << 9)    /* "no_fused_attention_bwd": attention backward and Q|K|V|C weight gradient as two kernels */
#define PMGT_OPT_STORE_LN_INPUT (1u << 10)           /* "store_ln_input": every LayerNorm site stores its input; default (bf16, hidden 256): x^ = (y - beta) / gamma from the OUTPUT */
#define PMGT_OPT_EAGER_REDUCE (1u << 11)             /* "eager_reduce": partial sums reduced by a launch per producer instead of one per gradient bucket */
#define PMGT_OPT_SIDE_STREAM_REDUCE (1u << 12)       /* "side_stream_reduce": ... on the engine's second stream (fork / join by events); measured neutral */
#define PMGT_OPT_UNFUSED_LN (1u << 13)               /* "unfused_ln": LayerNorm as its own launch after the streaming GEMM */
#define PMGT_OPT_ONE_BUCKET (1u << 14)               /* "one_bucket": the gradient-ready callback fires once per backward pass (whole buffer) */
#define PMGT_OPT_SMALL_ARENA (1u << 15)              /* "small_arena": (test) partial-sum arena sized for one producer: a batched reduction per producer */
#define PMGT_OPT_NO_ROLE_SPLIT_LN (1u << 16)         /* "no_role_split_ln": the 8-wave lockstep streaming kernels instead of the role-split ones of gemm_wsr.hip (K = N = 256 residual + LayerNorm; K = 512 plain / GELU / GELU' / residual) -- bit-identical results */
#define PMGT_OPT_UNFUSED_LN_BWD (1u << 18)           /* "unfused_ln_bwd": LayerNorm backward as its own launch behind the data-gradient GEMM that produces its dy (default, bf16 / hidden 256: epilogue of that GEMM) */
#define PMGT_OPT_LOCKSTEP_ATTENTION_BWD (1u << 19)   /* "lockstep_attention_bwd": fused attention backward with both (sequence, head) pairs of a step in the same phase instead of one barrier interval apart -- bit-identical results */
#define PMGT_OPT_SIDE_STREAM_WGRAD (1u << 20)        /* "side_stream_wgrad": the dense weight-gradient GEMMs of a layer on the engine's side stream, next to the data-gradient chain (same kernels, same reduction order: identical results; opt-in -- the cross-stream hand-offs cost more than the overlap gives at every batch size measured) */
#define PMGT_OPT_NO_CLS_ONLY_ATTENTION_BWD (1u << 21) /* "no_cls_only_attention_bwd": fused attention backward of the last (shortcut) layer without the skip of query tiles whose d ctx rows are zero -- identical results */
#define PMGT_OPT_NO_BETA_SKIP (1u << 22)            /* "no_beta_skip": beta == 1 (scripts/run_pmgt.sh:24) on the general fused kernels: Q / K projected, dot-product branch run and differentiated although it contributes exactly nothing (pmgt/pmgt/modeling_pmgt.py:519-521); default: skipped */
#define PMGT_OPT_NO_VC2_ATTENTION_BWD (1u << 23)    /* "no_vc2_attention_bwd": beta == 1 on the one-head-per-step vc_only backward instead of the two-heads-per-step form */
#define PMGT_OPT_NO_TILE_ATTENTION (1u << 17)        /* "no_tile_attention": S = 64 / head size 64 attention on the cooperative kernels (per-wave fragment loads) instead of the tile forms */

/* ---- which kernel families the calling thread has launched since the last reset (test instrumentation: a parity test at a given
 * size only covers a kernel if the dispatcher actually picked it).  Families: gemm_wsr, gemm_wsr_lnb, gemm_wsr512, gemm_ws, nt_big,
 * nt_big_gather, nt_big_128, nt_lnb, nt_tile, tn_big, tn_big_gather, tn_dma, tn_dma_gather, tn_tile, attn_tiles_fwd, attn_tiles_bwd,
 * qkvc_attn_fwd, attn_bwd_wgrad, f8_big, f8_tile, f8_wsr512, gemm_rowln, nt_lnf, embed_tok8, qkvc_attn_fwd_vc, attn_bwd_wgrad_vc, nt_vc, attn_bwd_wgrad_vc2 (the vc families: the beta == 1 forms, counted in addition to their general family).  Unknown name: -1. */
void pmgt_launch_trace_reset(void);
int64_t pmgt_launch_trace_count(const char* family);

/* ---- single-kernel entry points (unit/parity tests of each kernel against the oracle) ------------ */
/* Token order of the table-mode backward (the gather of pmgt/pmgt/utils.py:43-50 run in reverse: per-node sums of per-token gradients):
 * the stable sort of the M tokens by node id -- skeys [M] sorted ids, perm [M] token index at each sorted position (ties in index order),
 * seg_off [n_rows + 1] first sorted position of every id.  ids [M] int64 with values < n_rows; scratch_keys / scratch_vals [M] uint32;
 * temp: pmgt_op_seg_sort_temp_bytes(M) bytes.  Integer work: bit-exact against any stable sort. */
/* Measurement plumbing: `blocks` one-wave workgroups each write {shader-cycle counter, 100 MHz wall counter, XCC id, 1} to out [blocks][4]
 * (uint64).  Two probes on a stream around a timed region -> the shader clock the region sustained (bench.py: sustained_sclk_mhz). */
int pmgt_op_clock_probe(uint64_t* out, int blocks, void* stream);
int64_t pmgt_op_seg_sort_temp_bytes(int M);
int pmgt_op_seg_sort(const int64_t* ids, int M, int n_rows, uint32_t* scratch_keys, uint32_t* scratch_vals, uint32_t* skeys, uint32_t* perm,
                     int* seg_off, void* temp, int64_t temp_bytes, void* stream);
/* per-row absmax e4m3 quantisation (weights per output channel, activations per token): scale[r] = max|row| / 448 */
int pmgt_op_quant_rows_e4m3(int src_dtype, const void* src, int64_t lds, int rows, int cols, void* dst, int64_t ldd,
                            float* scale, void* stream);
/* C (bf16) = (A8 B8^T) * a_scale(row) * b_row_scale[n] + bias on the fp8 MFMA; a_rows = optional row gather on A */
int pmgt_op_gemm_nt_f8(const void* A, int64_t lda, const int64_t* a_rows, const float* a_row_scale, float a_scale,
                       const void* B, int64_t ldb, const float* b_row_scale, void* C, int64_t ldc, int M, int N, int K,
                       const float* bias, const int* m_dev, void* stream);
/* weight gradient with an e4m3 Q operand (feature-table rows): out = P^T (Q8 * q_scale), P bf16 */
int pmgt_op_gemm_tn_f8(const void* P, int64_t ldp, const void* Q8, int64_t ldq, float q_scale, const int64_t* q_rows, int M,
                       int N1, int N2, float* slab, float* out, int accumulate, const int* m_dev, void* stream);
/* fused projection + attention forward with the projection on the fp8 MFMA (d = 256): w8 [4d, d] e4m3, wscale [4d]; the layer
 * input either as bf16 x (quantised per row inside the kernel) or, x8 != NULL, as e4m3 rows + one scale per row */
int pmgt_op_qkvc_attention_fwd_f8(const void* x, const void* x8, const float* xscale, const void* w8, const float* wscale, const float* bias, const float* mask,
                                  void* qkvc, void* ctx, int n_seq, int S, int H, int dh, float beta, float drop_p,
                                  uint32_t site1, uint32_t site2, const uint64_t* rng, void* stream);
int pmgt_op_gemm_nt(int dtype, const void* A, int64_t lda, const int64_t* a_rows, const void* B, int64_t ldb, void* C,
                    int64_t ldc, int M, int N, int K, const float* bias, int epilogue, void* aux, int64_t ldaux,
                    const void* residual, int64_t ldr, float drop_p, uint32_t drop_site, const uint64_t* rng,
                    const int* m_dev, uint32_t path_opts, void* stream);
int64_t pmgt_op_gemm_tn_slab_elems(int dtype, int M, int N1, int N2, uint32_t path_opts);
int pmgt_op_gemm_tn(int dtype, const void* P, int64_t ldp, const void* Q, int64_t ldq, const int64_t* q_rows, int M,
                    int N1, int N2, float* slab, float* out, int accumulate, const int* m_dev, uint32_t path_opts, void* stream);
/* the same with the bias gradient (column sums of P; bias_slab: [512][N1] scratch) and the head-major row permutation of
 * the Q|K|V|C projection (perm_d = hidden size, perm_dh = head size; 0 = none) */
int pmgt_op_gemm_tn_bias(int dtype, const void* P, int64_t ldp, const void* Q, int64_t ldq, int M, int N1, int N2, float* slab,
                         float* out, float* bias_slab, float* bias_out, int perm_d, int perm_dh, uint32_t path_opts, void* stream);
/* column sums of Y [M, N]; slab: ceil(M / 96) * N floats of scratch */
int pmgt_op_colsum(int dtype, const void* Y, int64_t ldy, int M, int N, float* slab, float* out, void* stream);
int pmgt_op_layernorm_fwd(int dtype, const void* x, void* y, float* stats, const float* gamma, const float* beta,
                          int M, int d, float eps, float drop_p, uint32_t drop_site, const uint64_t* rng, void* stream);
/* part: [ceil(M/64)][3][d] scratch; dgamma_dbeta: [3*d] out = dgamma | dbeta | column sum of dx_drop (or dx) */
int pmgt_op_layernorm_bwd(int dtype, const void* dy, const void* x, const float* stats, const float* gamma, void* dx,
                          void* dx_drop, float* part, float* dgamma_dbeta, int M, int d, float in_drop_p,
                          uint32_t in_site, float out_drop_p, uint32_t out_site, const uint64_t* rng, void* stream);
/* One linear layer through the engine's dispatcher: bf16 with K <= 256 runs the weight-stationary streaming
 * kernel (gemm_ws.hip), everything else the tiled one; ln_out != NULL adds LayerNorm(C) (fused when N == 256). */
int pmgt_op_linear(int dtype, const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc, int M, int N, int K,
                   const float* bias, int epilogue, void* aux, int64_t ldaux, const void* residual, int64_t ldr, float drop_p,
                   uint32_t drop_site, const uint64_t* rng, void* ln_out, float* ln_stats, const float* ln_gamma,
                   const float* ln_beta, float ln_eps, uint32_t path_opts, void* stream);
/* dy = A B^T + residual, then the backward of the LayerNorm whose OUTPUT is y (x^ = (y - beta) / gamma; stats = its {mean, rstd}
 * rows): dx, dx_drop = dx * dropout mask (optional), dgamma | dbeta | column sums of the bf16 dx_drop (or dx) [3 N].  bf16.  One launch
 * where the role-split streaming kernel (K = N = 256, M >= 8192) or the 256 x 256 tile with the LayerNorm-backward phase (N = 256,
 * K % 64 == 0, >= 96 tiles) applies, else GEMM -> dy_tmp [M, N] -> LayerNorm backward (autograd through BertSelfOutput /
 * BertOutput, pmgt/pmgt/modeling_pmgt.py:293-294,322-325,332,371).  part: scratch of max(256, ceil(M / 64)) * 3 N floats. */
int pmgt_op_linear_ln_bwd(const void* A, int64_t lda, const void* B, int64_t ldb, int M, int N, int K, const void* residual, int64_t ldr,
                          const void* y, const float* stats, const float* gamma, const float* beta, void* dy_tmp, void* dx, void* dx_drop,
                          float drop_p, uint32_t drop_site, const uint64_t* rng, float* part, float* dgamma_dbeta_dbias,
                          uint32_t path_opts, void* stream);
/* ---- the compacted-row forms of the last-layer shortcut (the tail of the last encoder layer on the rows the loss reads): the launch is
 * sized for the capacity M on the host, the live row count min(M, *m_dev) is read on the device.  Rows >= the live count are neither
 * read nor written, and no sum counts them.  Each entry calls the host functions the engine calls at `sc` (csrc/engine.hip); the dispatch
 * of linear(), which is local to that file, is restated in ops/compact_rows.hip.  tests/test_compact_rows_gpu.py.
 * pmgt_op_linear with A rows through a_rows (logical row m reads A + a_rows[m] * lda; NULL: none), the residual row through the same list
 * (res_gather; needs a_rows) and m_dev: the dispatcher picks gemm_rowln, gemm_ws, gemm_wsr, gemm_wsr512 or the 128 x 128 tile, with the
 * standalone LayerNorm launch (which takes m_dev too) where LayerNorm is not fused. */
int pmgt_op_linear_rows(int dtype, const void* A, int64_t lda, const int64_t* a_rows, const void* B, int64_t ldb, void* C, int64_t ldc, int M,
                        int N, int K, const float* bias, int epilogue, void* aux, int64_t ldaux, const void* residual, int64_t ldr,
                        int res_gather, float drop_p, uint32_t drop_site, const uint64_t* rng, void* ln_out, float* ln_stats,
                        const float* ln_gamma, const float* ln_beta, float ln_eps, const int* m_dev, uint32_t path_opts, void* stream);
/* pmgt_op_layernorm_bwd with m_dev (x = the stored LayerNorm input); part: [ceil(M/64)][3][d] -- workgroups past the live rows write zeros */
int pmgt_op_layernorm_bwd_rows(int dtype, const void* dy, const void* x, const float* stats, const float* gamma, void* dx,
                               void* dx_drop, float* part, float* dgamma_dbeta, int M, int d, float in_drop_p, uint32_t in_site,
                               float out_drop_p, uint32_t out_site, const uint64_t* rng, const int* m_dev, void* stream);
/* pmgt_op_gemm_tn_bias with a row gather on Q, m_dev, accumulate (out and bias_out: +=) and the splits taken from m_for_splits instead of M
 * (the engine: max(256, M / 3)): slab holds pmgt_op_gemm_tn_slab_elems(dtype, m_for_splits, N1, N2) floats, bias_slab [512][N1] */
int pmgt_op_gemm_tn_bias_rows(int dtype, const void* P, int64_t ldp, const void* Q, int64_t ldq, const int64_t* q_rows, int M, int m_for_splits,
                              int N1, int N2, float* slab, float* out, float* bias_slab, float* bias_out, int accumulate, const int* m_dev,
                              uint32_t path_opts, void* stream);
/* Fused Q|K|V|C projection + attention forward (bf16; S = 32, dh = 32, hidden 128 or 256; returns -3 otherwise):
 * x [n_seq*S, d], w [4d, d] (rows q | k | v | c), bias [4d] fp32 -> qkvc [n_seq*S, 4d], ctx [n_seq*S, d]. */
int pmgt_op_qkvc_attention_fwd(const void* x, const void* w, const float* bias, const float* mask, void* qkvc, void* ctx,
                               int n_seq, int S, int H, int dh, float beta, float drop_p, uint32_t site1, uint32_t site2,
                               const uint64_t* rng, void* stream);
/* the same with layout / mode flags: bit 0 = qkvc written head-major ((head, matrix, w) columns), bit 1 = vc_only (beta == 1, H % 4 == 0: V and C
 * projected and stored only, cosine branch alone; the Q / K columns of qkvc are left untouched) */
int pmgt_op_qkvc_attention_fwd_ex(const void* x, const void* w, const float* bias, const float* mask, void* qkvc, void* ctx,
                                  int n_seq, int S, int H, int dh, float beta, float drop_p, uint32_t site1, uint32_t site2,
                                  const uint64_t* rng, int flags, void* stream);
int pmgt_op_attention_fwd(int dtype, const void* qkvc, const float* mask, void* ctx, float* probs, int n_seq, int S,
                          int H, int dh, float beta, float drop_p, uint32_t site1, uint32_t site2,
                          const uint64_t* rng, uint32_t path_opts, void* stream);
int pmgt_op_attention_bwd(int dtype, const void* qkvc, const float* mask, const void* dctx, void* dqkvc, int n_seq,
                          int S, int H, int dh, float beta, float drop_p, uint32_t site1, uint32_t site2,
                          const uint64_t* rng, uint32_t path_opts, void* stream);
/* Attention backward fused with the weight / bias gradient of the Q|K|V|C projection (bf16, S = 32, head size 32, hidden 128 or
 * 256; replaces pmgt_op_attention_bwd + the [M, 4d]^T [M, d] weight-gradient GEMM, i.e. autograd through
 * pmgt/pmgt/modeling_pmgt.py:429-433 and :435-526).  x = the layer input [n_seq * 32, d]; dqkvc as pmgt_op_attention_bwd;
 * slab [parts][4d * d] / bias_slab [parts][4d] (parts = pmgt_op_attention_bwd_wgrad_parts(H)) receive per-workgroup partial
 * sums in q | k | v | c row order, to be added up by the caller.  head_major: bit 0 = the column layout of qkvc / dqkvc, bit 1 = vc_only
 * (beta == 1: Q / K columns of qkvc are not read, dQ / dK columns of dqkvc not written, query / key rows of the partial sums are zeros). */
int pmgt_op_attention_bwd_wgrad_parts(int H);
int pmgt_op_attention_bwd_wgrad_vc2_parts(int H);      /* head_major bit 3: the two-barrier kernel; bit 2 (with bit 1): two heads per step; slab [vc2_parts][2d * d], bias_slab [vc2_parts][2d]: value | ctx_attention rows only */
int pmgt_op_attention_bwd_wgrad(const void* qkvc, const float* mask, const void* dctx, const void* x, void* dqkvc, float* slab,
                                float* bias_slab, int n_seq, int H, float beta, float drop_p, uint32_t site1, uint32_t site2,
                                const uint64_t* rng, int head_major, void* stream);

/* ---- row kernels of the embedding, the loss heads and the optimizer: each entry calls the host function the engine calls, with
 * the engine's dispatch (template instance by dtype / hidden size / modality count; the embed_tok8 kernel for bf16, phase 2, d = 256
 * with e_rows set, counted in the launch trace).  dtype: PMGT_DTYPE_F32 or PMGT_DTYPE_BF16 (activations); fp32 parameters. */

/* Modality mix + position + role + LayerNorm + dropout of PMGTEmbeddings from the projected feature rows on, and its backward.
 * phase 0: per token, E [M, nf d] (row e_rows[m] when e_rows != NULL);  table mode: phase 1 (rows = nodes) fwd writes a [M, nf] and
 * pre = F [M, d] = sum_k a_k e_k; bwd reads dF [M, d] (fp32 when dF_f32) and writes dE [M, nf d] + dWa / dba partials;  phase 2
 * (rows = tokens) fwd: x = E[e_rows[m]] (row stride d) + pos + role -> LayerNorm -> dropout, bwd: LayerNorm backward only (dF, dgamma /
 * dbeta partials).  pre == NULL in phase 2 (bf16, d = 256): the backward recomputes the pre-LayerNorm sum from E, pos and role.
 * part: [pmgt_op_embed_bwd_parts(M)][pmgt_op_embed_part_elems(d, nf)] = dgamma | dbeta | dWa (nf x nf d) | dba (padded to 4) per
 * workgroup.  Dropout on h0 (forward) and dh0 (backward) with (rng, drop_p, drop_site) as the other entries; rng == NULL: none. */
typedef struct pmgt_embed_args {
    int dtype, phase, M, S, d, nf;
    const void* E;
    const int64_t* e_rows;
    const float *Wa, *ba, *pos, *role, *gamma, *beta;
    float eps;
    float* a;
    void* pre;
    float* stats;
    void* h0;
    float drop_p;
    uint32_t drop_site;
    const uint64_t* rng;
    const void* dh0;
    void* dE;
    void* dF;
    int dF_f32;
    float* part;
} pmgt_embed_args;
int pmgt_op_embed_mix_fwd(const pmgt_embed_args* args, void* stream);
int pmgt_op_embed_mix_bwd(const pmgt_embed_args* args, void* stream);
int pmgt_op_embed_part_elems(int d, int nf);
int pmgt_op_embed_bwd_parts(int M);
/* dpos [max_pos, d] = possum [S, d] (zero rows for s >= S), drole [2, d] = {possum[0], sum_{s >= 1} possum[s]}; accumulate: += */
int pmgt_op_pos_role_finish(const float* possum, int S, int d, int max_pos, float* dpos, float* drole, int accumulate, void* stream);
/* out [n_rows, cols] (row stride cols) = per-node sums of src [M, cols] (row stride ld) over the segments of pmgt_op_seg_sort's
 * skeys / perm / seg_off; zero rows for empty segments.  (in_dtype, out_dtype): (F32, F32), (BF16, BF16) or (BF16, F32).
 * part: pmgt_op_seg_part_elems(M, cols) floats of scratch. */
int64_t pmgt_op_seg_part_elems(int M, int cols);
int pmgt_op_seg_sum(int in_dtype, int out_dtype, const void* src, int64_t ld, const uint32_t* skeys, const uint32_t* perm, const int* seg_off,
                    int M, int n_rows, int cols, void* out, float* part, void* stream);
/* off [B + 1] = exclusive prefix sum of num_pairs [B] */
int pmgt_op_pair_offsets(const int64_t* num_pairs, int B, int* off, void* stream);
/* row-major compaction of tgt_full [B, S] (-1 = not masked): rows[k] = (seq_off + b) * S + s, tids[k] = tgt_full[b, s], *count */
int pmgt_op_nfr_compact(const int64_t* tgt_full, int B, int S, int seq_off, int64_t* rows, int64_t* tids, int* count, void* stream);
/* NFR masking with the device RNG (site ids 5 and 6 of layer -1): ids [B, S] -> masked_ids [B, S], tgt_full [B, S] (-1 = not masked).
 * Position 0 and padding (id 0) are never touched; replaced ids lie in [2, n_nodes + 2).  Integer work: bit-exact against a restatement. */
int pmgt_op_nfr_generate(const int64_t* ids, int B, int S, int n_nodes, float random_ratio, float mask_ratio, const uint64_t* rng,
                         int64_t* masked_ids, int64_t* tgt_full, void* stream);
/* rows the loss reads from the last layer, in compact order: CLS rows of the B targets (b * S), of the P pairs ((B + p) * S), then
 * nfr_rows[0 .. *nfr_count); *count = B + P + *nfr_count.  rows: capacity B + P + B * max(S - 1, 1), which *nfr_count must not exceed
 * (less B + P).  inv (optional, [n_tokens] ints): token row -> compact row, -1 elsewhere; every listed row must be < n_tokens. */
int pmgt_op_build_need_rows(int B, int P, int S, const int64_t* nfr_rows, const int* nfr_count, int64_t* rows, int* count, int* inv,
                            int64_t n_tokens, void* stream);
/* Keep decisions of the dropout RNG, out [rows, cols] bytes (1 = kept): what every dropout-bearing kernel draws for element (row, col) of
 * site `site` at rng = {seed, step} (csrc/common.h: one hash pair per (row, col / 4), 16-bit lane col % 4 against (uint32)(p 2^32) >> 16);
 * p <= 0: all kept, rng not read. */
int pmgt_op_dropout_keep(const uint64_t* rng, float p, uint32_t site, int rows, int cols, uint8_t* out, void* stream);
/* graph-structure loss: h [(B + P) rows of CLS, cls_stride apart, d], off [B + 1] pair offsets, labels [P] -> logits [P],
 * loss_part [B] (loss_i / B) and, dh != NULL, the gradient of the mean loss written to the CLS rows of dh (other rows untouched) */
int pmgt_op_gsr(int dtype, const void* h, void* dh, int B, int S, int d, int64_t cls_stride, const int* off, const float* labels,
                float* logits, float* loss_part, void* stream);
/* pred [cap, sum F] in, d loss_nfr / d pred out for rows < *count; tables[m] [N + 2, F[m]] (e4m3 bytes times scales[m] when tables_f8);
 * sse_part [pmgt_op_nfr_diff_parts(cap)][4] squared-error partials per modality */
int pmgt_op_nfr_diff_parts(int cap);
int pmgt_op_nfr_diff(int dtype, void* pred, const int64_t* tids, const int* count, int cap, int nf, const int* F, const void* const* tables,
                     int tables_f8, const float* scales, float* sse_part, void* stream);
/* out [3] = {gsr + nfr, gsr, nfr}; nfr = mean over modalities of sse_m / (count F[m]) (NaN for count 0); count_out: copy of *count */
int pmgt_op_loss_finish(const float* gsr_part, int B, const float* sse_part, int nparts, const int* count, int nf, const int* F, int with_nfr,
                        float* out, int* count_out, void* stream);
/* dst[rows[k], :d] = src[k, :d] (add: +=) for k < *count */
int pmgt_op_scatter_rows(int dtype, const void* src, const int64_t* rows, const int* count, int cap, int d, void* dst, int add, void* stream);
/* global-norm clip (max_norm <= 0: off) + AdamW over flat fp32 buffers; step: device counter, incremented; scal [4] = clip coefficient,
 * lr / bc1, 1 / sqrt(bc2), gradient norm; part: 1024 floats of scratch */
int pmgt_op_adamw(float* p, const float* g, float* m, float* v, const uint8_t* decay, int64_t n, float lr, float wd, float b1, float b2,
                  float eps, float max_norm, int64_t* step, float* scal, float* part, void* stream);
/* the same with a learning-rate schedule (pmgt_lr_schedule, pmgt_capi.h) evaluated on the device from *step; scal is [8] here, laid out as
 * pmgt_optimizer_step_scheduled states (lr_t = lr * lambda of the steps completed before this one) */
int pmgt_op_adamw_scheduled(float* p, const float* g, float* m, float* v, const uint8_t* decay, int64_t n, float lr, float wd, float b1,
                            float b2, float eps, float max_norm, int64_t* step, float* scal, float* part, const pmgt_lr_schedule* sched,
                            void* stream);
/* the same behind the step guard (pmgt_step_guard, pmgt_capi.h); sched may be NULL (constant lr: pmgt_op_adamw bit for bit on an applied
 * step); scal [8] of the same layout */
int pmgt_op_adamw_guarded(float* p, const float* g, float* m, float* v, const uint8_t* decay, int64_t n, float lr, float wd, float b1,
                          float b2, float eps, float max_norm, int64_t* step, float* scal, float* part, const pmgt_lr_schedule* sched,
                          const pmgt_step_guard* guard, void* stream);
/* global-norm clip (max_norm <= 0: off) + SGD over a flat fp32 buffer: torch.optim.SGD without momentum, with COUPLED weight decay where the
 * decay byte is 1, after clip_grad_norm_ and under a LambdaLR stepped per optimizer step (the reference's --optim sgd).  Three launches: the
 * norm partials of pmgt_op_adamw, the prepare lane of pmgt_op_adamw_guarded (so clip, lr_t = lr * lambda(*step), the guard's decision, its
 * counters and its log row are that entry's, bit for bit; lr_t is pmgt_op_lr_schedule's value), one update.  sched NULL: constant rate;
 * guard NULL: unguarded.  scal [8]: [0] clip, [1] lr_t, [2] 1, [3] pre-clip norm, [4] lr_t, [5] skipped flag (guarded only), [6..7]
 * untouched.  An applied step increments *step; a skipped one leaves *step and every byte of p alone, writes [0] = 0, [3] = the non-finite
 * norm, [4] = the rate it would have used, and leaves [1] and [2] unwritten.  Per element, in fp32 with every product and sum rounded (no
 * FMA): gc = g clip; d = decay ? gc + wd p : gc; p = p - lr_t d.  p and g need 4-byte alignment only; n == 0 runs the prepare lane alone.
 * -2 before any launch: a NULL p, g, decay, step, scal or part; n < 0; lr, wd or max_norm not finite; what pmgt_op_adamw_guarded refuses
 * of a schedule or guard that is given. */
int pmgt_op_sgd(float* p, const float* g, const uint8_t* decay, int64_t n, float lr, float wd, float max_norm, int64_t* step, float* scal,
                float* part, const pmgt_lr_schedule* sched, const pmgt_step_guard* guard, void* stream);
/* Global-norm clip + AdamW over up to PMGT_ADAM_MAX_SEGMENTS disjoint flat fp32 buffers AS ONE OPTIMIZER: the norm is taken over all
 * segments (the partials of the plain step's own norm kernel per segment, summed in fp64 by the prepare lane), there is one clip
 * coefficient, one increment of *step and one pair of bias corrections.  Per segment both the step size and the decay rate are multiplied
 * by lr_scale (an encoder fine-tuned through a head at a learning rate of its own); lr_scale = 0 leaves that segment's p untouched bit
 * for bit while its m and v move.  With ONE segment and lr_scale == 1 the call gives the plain entry's bits (p, m, v, step, scal[0..3]).
 * scal [8]: [0..3] as the plain entry, [4] = lr; part [count * 1024] floats of scratch.  An empty segment (n = 0) is skipped.  Launches:
 * one norm launch and one update launch per non-empty segment, one prepare launch; no sync, no allocation, capturable.
 * Refused (-2) before any launch: count outside [1, PMGT_ADAM_MAX_SEGMENTS], a NULL pointer, n < 0, lr_scale not finite or negative. */
#define PMGT_ADAM_MAX_SEGMENTS 8
typedef struct pmgt_adam_segment {
    float* p;
    const float* g;
    float* m;
    float* v;
    const uint8_t* decay;
    int64_t n;
    float lr_scale;
} pmgt_adam_segment;
int pmgt_op_adamw_segments(const pmgt_adam_segment* segments, int count, float lr, float wd, float b1, float b2, float eps, float max_norm,
                           int64_t* step, float* scal, float* part, void* stream);
/* pmgt_op_adamw_segments with the options of the single-buffer entries: the same segments stepped as ONE optimizer (one norm over all of
 * them, one clip coefficient, one *step, a rate per segment), by AdamW or SGD, optionally under a learning-rate schedule and behind the
 * step guard.  sched NULL: constant rate; guard NULL: unguarded.  PMGT_OPTIM_ADAMW with neither is pmgt_op_adamw_segments bit for bit
 * (p, m, v, step, scal[0..4]); with ONE segment at lr_scale 1, PMGT_OPTIM_ADAMW is pmgt_op_adamw_guarded and PMGT_OPTIM_SGD is pmgt_op_sgd
 * bit for bit, counters and log row included.
 * The prepare lane is the single-buffer entries' own code over the partials of every segment (a lane adds segment 0's, then segment 1's,
 * ..., in fp64): lr_t = lr * lambda(*step) is pmgt_op_lr_schedule's value, and scal [8] has the layout pmgt_op_adamw_guarded and pmgt_op_sgd
 * document ([0] clip, [1] lr_t / bc1, [2] 1 / sqrt(bc2), [3] pre-clip joint norm, [4] lr_t, [5] skipped flag (guarded only), [6..7]
 * untouched; SGD runs the lane with beta1 = beta2 = 0, so [1] = lr_t and [2] = 1).  An applied step increments *step; a skipped one leaves
 * *step and every byte of every segment's p, m and v alone, writes [0] = 0, [3] = the non-finite norm, [4] = the rate it would have used.
 * Per segment: AdamW as pmgt_op_adamw_segments states it, with the step size scal[1] * lr_scale and the decay rate the fp32 product
 * scal[4] * lr_scale; SGD as pmgt_op_sgd states it at lr_t = scal[4] * lr_scale (one rounded fp32 product), m and v may be NULL and are
 * never read, p and g need 4-byte alignment only (a range of a larger buffer takes the 16-byte body when p and g share their alignment).
 * lr_scale = 0: AdamW leaves p untouched while m and v move; SGD with finite gradients leaves p untouched.
 * part [count * 1024] floats of scratch.  An empty segment (n = 0) is skipped.  Launches: one norm launch and one update launch per
 * non-empty segment, one prepare launch; no sync, no allocation, no atomics, capturable.
 * Refused (-2) before any launch, nothing written: what pmgt_op_adamw_segments refuses (under SGD a NULL m or v is accepted); an optim that
 * is neither value; lr, wd or max_norm not finite; what pmgt_op_adamw_guarded refuses of a schedule or guard that is given. */
#define PMGT_OPTIM_ADAMW 0
#define PMGT_OPTIM_SGD   1
int pmgt_op_step_segments(const pmgt_adam_segment* segments, int count, int optim, float lr, float wd, float b1, float b2, float eps,
                          float max_norm, int64_t* step, float* scal, float* part, const pmgt_lr_schedule* sched,
                          const pmgt_step_guard* guard, void* stream);
/* The two-way glue between an encoder output [n][S][d] in the engine dtype (PMGT_DTYPE_F32 or PMGT_DTYPE_BF16) and the fp32 rows [n][d] a head
 * reads and differentiates.  Gather: x[p][:] = (float) last_hidden[p][0][:], the CLS state of sequence p.  Scatter: d_last [n][S][d] is
 * written WHOLE -- token 0 of sequence p gets d_item[p] (fp32 -> bf16 round-to-nearest-even), every other element +0.0.  16-byte accesses
 * where d is a multiple of 8, element by element otherwise.  One launch each.  Refused (-2): a NULL pointer, n, S or d below 1, a dtype
 * that is neither, n S d beyond 2^40. */
int pmgt_op_cls_gather(int dtype, const void* last_hidden, int64_t n, int S, int d, float* x, void* stream);
int pmgt_op_cls_scatter(int dtype, const float* d_item, int64_t n, int S, int d, void* d_last, void* stream);
/* The append entry of the validation metrics in pmgt_capi.h, on ready scores: no sigmoid, everything else the same (negative, subnormal, infinite and NaN scores reach
 * the key function as they are) */
int pmgt_op_eval_append_scores(void* workspace, int64_t capacity, const float* scores, const float* labels, const float* loss, int64_t offset,
                               int64_t n, int64_t n_targets, void* stream);
/* size switch of pmgt_eval_reduce: up to this many predictions one workgroup sorts in LDS (it is that workgroup's element count too);
 * more take the multi-tile radix path */
int pmgt_op_eval_small_max(void);
/* out [n] = lr * lambda of steps first_step .. first_step + n - 1: the device function of the scheduled step, one launch */
int pmgt_op_lr_schedule(const pmgt_lr_schedule* sched, float lr, int64_t first_step, int n, float* out, void* stream);
/* weight mirror: per descriptor, W = params[src ..] [rows, cols] copied as dtype to mirror[dst ..], transposed to mirror[dst_t ..] and
 * transposed with head-major columns to mirror[dst_t_hm ..] (offsets in elements, -1 = none); tile_start = first 32 x 32 tile of the
 * descriptor in the launch, total_tiles = all of them.  desc is a host array, copied to the device by the entry (synchronous). */
typedef struct pmgt_mirror_desc {
    int64_t src;
    int rows, cols;
    int64_t dst, dst_t, dst_t_hm;
    int hm_d, hm_dh;
    int tile_start;
} pmgt_mirror_desc;
int pmgt_op_mirror(int dtype, const float* params, void* mirror, const pmgt_mirror_desc* desc, int ndesc, int total_tiles, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PMGT_OPS_H */
