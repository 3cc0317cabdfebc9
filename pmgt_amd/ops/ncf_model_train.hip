// Training of the reference's stand-alone NCF class (pmgt/ncf/models.py:14-154, the class ncf.py restates; pmgt_ncf_model_train_grad of
// include/pmgt_capi.h): loss, logits and the gradient of the mean BCE-with-logits loss with respect to every tensor the model's kind trains,
// for n (user, item, label) pairs, in TWO launches.  Kept out of csrc/ for ncf_train.hip's reason.  The pair-major product forms, the roles
// rank / zero / weight / rows and the chain policies are stated in pair_train_tile.h; this file's products are Chain::FOUR without an
// activation in the epilogue (the LayerNorm comes first), and the predict layer's dot follows the same rule: FOUR sums a lane, factor f
// into sum f & 3, joined as (a + b) + (c + d).
//
// WHICH CASES RUN HERE.  A model WITHOUT LayerNorm of kind MLP / NeuMF-end (NeuMF-pre trains as NeuMF-end) is the head ncf_train.hip trains
// over a table: the entry hands it to pmgt_ncf_train_grad / _table / _dropout on the same buffers (the layouts agree), so those bits are
// that file's.  The kernels below cover the LayerNorm layer  h_(l+1) = relu(LN_l(m_l (W_l h_l + b_l)))  and kind GMF
// z = wp . (m_g (gu gi)) + bp, which is the degenerate path with no layer: no MLP tensor is read.
//
// LAUNCH 1, ncf_model_pairs_kernel: the roles rank (by user id and by item id) and zero (the embedding gradients and, as a second range,
// the gradient of embed_item_MLP when it is trained), and
//   tile   32 pairs a workgroup of 4 waves.  Per layer: the MFMA product y_l = m_l (W_l x + b_l) (the DROPPED pre-LayerNorm value is
//          stored), a barrier, then ROW WORK: one wave owns a pair's row (at most 256 floats, 4 a lane at lane + 64 j), reduces with a
//          shuffle butterfly in fp32 and stores (mean, rstd) and h_(l+1) = relu(xhat gamma + beta).  Then the GMF product, the predict
//          layer, the loss and dlogit.  Back: row work g = dh (h > 0) (stored: gamma / beta read g and xhat),
//          dy = m_l LNbwd(g) = m_l rstd ((g gamma - mean(g gamma)) - xhat mean(g gamma xhat)), a barrier, the MFMA data product
//          dh_(l-1) = dy W_l, down to dx [n][2 d] = m_e (dy_0 W_0).  The layer mask is drawn again on the way back; nothing of it is stored.
// LAUNCH 2, ncf_model_grads_kernel: the roles weight and rows (ncf_train.hip's column groups, the user half of dx only when the kind has
// an MLP branch), and
//   cols   64 columns of one layer a workgroup: d gamma = sum_p g xhat and d beta = sum_p g, xhat recomputed from the stored y and
//          (mean, rstd) by launch 1's sequence of operations (the file is compiled without contraction, so the bits agree); wave a sums
//          the pairs a, a + 4, .. in order and the four partial sums are added as (w0 + w1) + (w2 + w3)
// The same inputs give the same bits, on other buffers and another workspace too.
// DROPOUT: ncf_train.hip's sites and RNG: emb on the 16-byte x loads of layer 0 (drawn again by the weight task of layer 0 and by the last
// data gradient), layer l on y_l before its store (drawn again for dy_l), gmf on the GMF product.  A site whose p is 0 draws nothing; with
// every p 0 no dropout instantiation is launched.
#include <climits>
#include <cmath>

#include "pair_train_tile.h"

#pragma clang fp contract(off)

namespace pmgt {

static constexpr int NM_MAX_LAYERS = PMGT_NCF_MAX_LAYERS, NM_MAX_TASKS = NM_MAX_LAYERS + 1;

struct NmLayer {
    const float *w, *b, *gamma, *beta;      // [out][2 out], [out] x 3
    float *y, *h, *g, *dz;                  // workspace [n][out]: m (W x + b); relu(LN(y)); dh, then dh (h > 0); d loss / d (W x + b)
    float* stat;                            // workspace [n][2]: (mean, rstd) of y's row
    int out;
};

struct NmPairsArgs {
    NmLayer layer[NM_MAX_LAYERS];
    const float *u_mlp, *table, *gu, *gi, *wp, *bp;
    const int64_t *users, *items;
    const float* labels;
    float *dx, *gprod, *ggu, *ggi, *pz;      // workspace: [n][2 d], [n][F] x 3, [n][2] = (dlogit, loss of the pair)
    int *order_u, *order_i;
    float* logits;                           // [n] or NULL
    float* zero_base;                        // the embedding gradients
    int64_t zero_vec4;
    float* zero2_base;                       // the gradient of embed_item_MLP (trained), a second range
    int64_t zero2_vec4;                      // 0: no second range
    float eps;
    int n, d, factor, num_layers, gmf, tiles, rank_blocks, zero_blocks;      // num_layers 0: kind GMF
};

struct NmJob {           // cols: d gamma and d beta of one layer
    const float *g, *y, *stat;
    float *ggamma, *gbeta;
    int W, first;
};

typedef pmgt_ncf_dropout NmDrop;

struct NmGradsArgs {
    PairTask task[NM_MAX_TASKS];
    NmJob job[NM_MAX_LAYERS];
    const int64_t *users, *items;
    const int *order_u, *order_i;
    const float *dx, *ggu, *ggi;
    float *g_u_mlp, *g_gu, *g_gi, *g_table, *loss;      // g_table: the gradient of a trained embed_item_MLP, else NULL
    int n, d, factor, gmf, mlp, ntasks, njobs, weight_blocks, col_blocks, row_blocks;
};

template <bool DROP>
__global__ __launch_bounds__(PAIR_THREADS) void ncf_model_pairs_kernel(NmPairsArgs a, NmDrop dr) {
    __shared__ float s_dl[PAIR_TILE];
    __shared__ int64_t s_ids[PAIR_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = pair_wave_index(), n = a.n;
    int bid = blockIdx.x;
    if (bid >= a.tiles + 2 * a.rank_blocks) {                // ---- zero: the embedding gradients, whole, and embed_item_MLP's
        pair_zero<true>(bid - a.tiles - 2 * a.rank_blocks, a.zero_blocks, a.zero_base, a.zero_vec4, a.zero2_base, a.zero2_vec4, tid);
        return;
    }
    if (bid >= a.tiles) {                                    // ---- rank: the stable order by id, counted
        pair_rank(bid - a.tiles, a.rank_blocks, n, a.users, a.items, a.order_u, a.order_i, s_ids, tid);
        return;
    }
    // ---- tile: forward and data gradient of 32 pairs
    const int d = a.d, F = a.factor, L = a.num_layers;
    const int pl = lane & 31, h = lane >> 5;
    const int pair = bid * PAIR_TILE + pl;
    const bool valid = pair < n;
    const int64_t uid = valid ? a.users[pair] : 0, iid = valid ? a.items[pair] : 0;
    DropKey kemb = pair_drop_off(), kgmf = pair_drop_off();
    if constexpr (DROP) {
        if (L) kemb = make_drop_key(DropCfg{dr.rng, dr.p_emb, NCF_SITE_EMB});
        if (a.gmf) kgmf = make_drop_key(DropCfg{dr.rng, dr.p_emb, NCF_SITE_GMF});
    }
    for (int l = 0; l < L; ++l) {
        const NmLayer& ly = a.layer[l];
        const int M = ly.out;
        DropKey klay = pair_drop_off();
        if constexpr (DROP) klay = make_drop_key(DropCfg{dr.rng, dr.p_layer[l], NCF_SITE_LAYER + (uint32_t)l});
        if (l == 0)
            pair_linear<Chain::FOUR, false, DROP>(ly.w, ly.b, d, 2 * d, a.u_mlp + uid * d, d, a.table + iid * d, valid, ly.y + (int64_t)pair * d,
                                                  wave, lane, kemb, klay, pair);
        else
            pair_linear<Chain::FOUR, false, DROP>(ly.w, ly.b, M, 2 * M, a.layer[l - 1].h + (int64_t)pair * 2 * M, 2 * M, nullptr, valid,
                                                  ly.y + (int64_t)pair * M, wave, lane, pair_drop_off(), klay, pair);
        __syncthreads();
        const float inv = 1.f / (float)M;
        for (int pp = wave; pp < PAIR_TILE; pp += PAIR_WAVES) {  // row work: LayerNorm and ReLU, a wave a row
            const int pr = bid * PAIR_TILE + pp;
            if (pr >= n) break;                              // (uniform per wave)
            const float* yrow = ly.y + (int64_t)pr * M;
            float v[4], c[4], s = 0.f, q = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = lane + 64 * j;
                v[j] = f < M ? yrow[f] : 0.f;
                s += v[j];
            }
            const float mean = pair_wave_sum(s) * inv;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c[j] = lane + 64 * j < M ? v[j] - mean : 0.f;
                q += c[j] * c[j];
            }
            const float rstd = 1.f / sqrtf(pair_wave_sum(q) * inv + a.eps);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = lane + 64 * j;
                if (f < M) ly.h[(int64_t)pr * M + f] = relu_keep_nan((c[j] * rstd) * ly.gamma[f] + ly.beta[f]);
            }
            if (lane == 0) ly.stat[(int64_t)pr * 2] = mean, ly.stat[(int64_t)pr * 2 + 1] = rstd;
        }
        __syncthreads();
    }
    const float* feat = L ? a.layer[L - 1].h : nullptr;      // [n][F]
    const float* wp_mlp = a.wp + (a.gmf ? F : 0);
    if (wave == 0) {                                         // predict layer, loss, dlogit: a pair on lanes p and p + 32, half the factors each
        float s4[4] = {0.f, 0.f, 0.f, 0.f};                  // FOUR sums a lane, factor f into sum f & 3: chains of F / 8 terms, not F / 2
        if (valid) {
            const int half = F >> 1;                         // (a multiple of 4: one draw per 4 factors)
            if (a.gmf) {
                const float* gu = a.gu + uid * F;
                const float* gi = a.gi + iid * F;
                for (int f = h * half; f < (h + 1) * half; f += 4) {
                    float mk[4] = {1.f, 1.f, 1.f, 1.f};
                    if constexpr (DROP) {
                        if (kgmf.on) drop_mul4(kgmf, (uint32_t)pair, (uint32_t)(f >> 2), mk);
                    }
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float g = gu[f + e] * gi[f + e];
                        if constexpr (DROP) g *= mk[e];
                        a.gprod[(int64_t)pair * F + f + e] = g;
                        s4[e] = fmaf(a.wp[f + e], g, s4[e]);
                    }
                }
            }
            if (L) {
                const float* hl = feat + (int64_t)pair * F;
                for (int f = h * half; f < (h + 1) * half; f += 4)
#pragma unroll
                    for (int e = 0; e < 4; ++e) s4[e] = fmaf(wp_mlp[f + e], hl[f + e], s4[e]);
            }
        }
        float s = (s4[0] + s4[1]) + (s4[2] + s4[3]);
        s += __shfl_xor(s, 32, 64);
        if (h == 0) {
            float dl = 0.f;
            if (valid) {
                const float z = s + a.bp[0];
                float loss;
                pair_bce<false>(z, a.labels[pair], n, dl, loss);
                if (a.logits) a.logits[pair] = z;
                a.pz[(int64_t)pair * 2] = dl;
                a.pz[(int64_t)pair * 2 + 1] = loss;
            }
            s_dl[pl] = dl;
        }
    }
    __syncthreads();
    if (a.gmf) {
        for (int e = tid; e < PAIR_TILE * F; e += PAIR_THREADS) {    // the per-pair GMF gradients
            const int pp = e / F, f = e - pp * F, pr = bid * PAIR_TILE + pp;
            if (pr >= n) continue;
            const int64_t at = (int64_t)pr * F + f;
            float dg = s_dl[pp] * a.wp[f];
            if constexpr (DROP) {
                if (kgmf.on) dg *= drop_mul1(kgmf, (uint32_t)pr, (uint32_t)f);
            }
            a.ggu[at] = dg * a.gi[a.items[pr] * F + f];
            a.ggi[at] = dg * a.gu[a.users[pr] * F + f];
        }
    }
    for (int l = L - 1; l >= 0; --l) {
        const NmLayer& ly = a.layer[l];
        const int M = ly.out;
        DropKey klay = pair_drop_off();
        if constexpr (DROP) klay = make_drop_key(DropCfg{dr.rng, dr.p_layer[l], NCF_SITE_LAYER + (uint32_t)l});
        const float inv = 1.f / (float)M;
        for (int pp = wave; pp < PAIR_TILE; pp += PAIR_WAVES) {  // row work: g = dh (h > 0), dy = m LNbwd(g)
            const int pr = bid * PAIR_TILE + pp;
            if (pr >= n) break;
            const int64_t row = (int64_t)pr * M;
            const float mean = ly.stat[(int64_t)pr * 2], rstd = ly.stat[(int64_t)pr * 2 + 1], dl = s_dl[pp];
            float gp[4], xh[4], s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = lane + 64 * j;
                gp[j] = xh[j] = 0.f;
                if (f < M) {
                    xh[j] = (ly.y[row + f] - mean) * rstd;
                    const float dh = l == L - 1 ? dl * wp_mlp[f] : ly.g[row + f];
                    const float g = ly.h[row + f] > 0.f ? dh : 0.f;
                    ly.g[row + f] = g;
                    gp[j] = g * ly.gamma[f];
                }
                s1 += gp[j];
                s2 += gp[j] * xh[j];
            }
            const float m1 = pair_wave_sum(s1) * inv, m2 = pair_wave_sum(s2) * inv;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = lane + 64 * j;
                if (f < M) {
                    float dy = rstd * ((gp[j] - m1) - xh[j] * m2);
                    if constexpr (DROP) {
                        if (klay.on) dy *= drop_mul1(klay, (uint32_t)pr, (uint32_t)f);
                    }
                    ly.dz[row + f] = dy;
                }
            }
        }
        __syncthreads();
        if (l > 0)
            pair_linear_bwd<Chain::FOUR, DROP>(ly.w, M, 2 * M, 2 * M, ly.dz + (int64_t)pair * M, nullptr, valid,
                                               a.layer[l - 1].g + (int64_t)pair * 2 * M, wave, lane, 1.f, pair_drop_off(), pair);
        else
            pair_linear_bwd<Chain::FOUR, DROP>(ly.w, d, 2 * d, 2 * d, ly.dz + (int64_t)pair * d, nullptr, valid, a.dx + (int64_t)pair * 2 * d, wave,
                                               lane, 1.f, kemb, pair);
        __syncthreads();
    }
}

// DROP: the weight task of layer 0 gathers its B operand from the tables and applies the emb mask to it, drawn again per element
template <bool DROP>
// 7 waves a SIMD (72 VGPRs), the occupancy of the DROP instantiations before the weight role was shared (68 VGPRs; the plain ones had 80 and 6
// waves): unbounded, the DROP instantiations take 73, one over; the plain ones need 67 either way
__global__ __launch_bounds__(PAIR_THREADS, 7) void ncf_model_grads_kernel(NmGradsArgs a, NmDrop dr) {
    __shared__ float s_acc[PAIR_WAVES][16][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = pair_wave_index(), n = a.n;
    int bid = blockIdx.x;
    if (bid >= a.weight_blocks + a.col_blocks) {             // ---- rows: segment sums of the per-pair embedding gradients in pair order
        const PairRun r = pair_run(bid - a.weight_blocks - a.col_blocks, a.row_blocks, wave, n, a.users, a.items, a.order_u, a.order_i);
        if (!r.start) return;
        const int kind = r.kind;
        const int d = a.d, F = a.factor;
        const int Fg = a.gmf ? F : 0, du = a.mlp ? d : 0;
        const int width = kind ? Fg + (a.g_table ? d : 0) : du + Fg;
        for (int c = lane; c < width; c += 64) {
            const float* src;                                // the per-pair rows, `sw` floats apart
            float* dst;                                      // the table's rows, `w` floats wide
            int sw, w, cc;
            if (kind) {
                if (c < Fg) { src = a.ggi; dst = a.g_gi; sw = w = F; cc = c; }
                else { src = a.dx + d; dst = a.g_table; sw = 2 * d; w = d; cc = c - Fg; }
            }
            else if (c < du) { src = a.dx; dst = a.g_u_mlp; sw = 2 * d; w = d; cc = c; }
            else { src = a.ggu; dst = a.g_gu; sw = w = F; cc = c - du; }
            dst[r.id * w + cc] = pair_run_sum(r, n, src, sw, cc);
        }
        return;
    }
    if (bid >= a.weight_blocks) {                            // ---- cols: d gamma and d beta of 64 columns, the pairs in order
        bid -= a.weight_blocks;
        int ji = 0;
        for (int i = 1; i < a.njobs; ++i)
            if (bid >= a.job[i].first) ji = i;
        const NmJob& jb = a.job[ji];
        const int col = (bid - jb.first) * 64 + lane, W = jb.W;
        const bool ok = col < W;
        float sg = 0.f, sb = 0.f;
        for (int p = wave; p < n; p += PAIR_WAVES) {
            if (!ok) break;
            const int64_t at = (int64_t)p * W + col;
            const float g = jb.g[at];
            sg += g * ((jb.y[at] - jb.stat[(int64_t)p * 2]) * jb.stat[(int64_t)p * 2 + 1]);
            sb += g;
        }
        s_acc[wave][0][lane] = sg;
        s_acc[wave][1][lane] = sb;
        __syncthreads();
        if (wave == 0 && ok) {
            jb.ggamma[col] = (s_acc[0][0][lane] + s_acc[1][0][lane]) + (s_acc[2][0][lane] + s_acc[3][0][lane]);
            jb.gbeta[col] = (s_acc[0][1][lane] + s_acc[1][1][lane]) + (s_acc[2][1][lane] + s_acc[3][1][lane]);
        }
        return;
    }
    // ---- weight: one 32 x 32 block of dW = dz^T x, the pairs in order
    pair_weight_block<DROP, true>(a.task, a.ntasks, bid, n, a.loss, DropCfg{dr.rng, dr.p_emb, NCF_SITE_EMB}, s_acc, tid, lane, wave);
}

struct NmShape {
    int F, L, d, gmf, mlp, ln, table;      // L: the MLP layers the kind reads (kind GMF: 0); table: embed_item_MLP is trained
    int64_t user_num, item_num;
};

static constexpr int NM_OFF_WP = 3 + 4 * NM_MAX_LAYERS, NM_OFF_BP = NM_OFF_WP + 1, NM_OFF_TABLE = NM_OFF_WP + 2;
static_assert(NM_OFF_TABLE + 1 == PMGT_NCF_MODEL_TENSORS, "the slot count of pmgt_ncf_model_layout");

static int nm_shape(int factor_num, int num_layers, int kind, int use_layer_norm, int train_items, int64_t user_num, int64_t item_num,
                    const char* who, NmShape* s) {
    PMGT_CHECK(factor_num == 8 || factor_num == 16 || factor_num == 32 || factor_num == 64, -2, "%s: factor_num = %d, covered: 8, 16, 32, 64", who,
               factor_num);
    PMGT_CHECK(num_layers >= 1 && num_layers <= NM_MAX_LAYERS, -2, "%s: num_layers = %d outside [1, %d]", who, num_layers, NM_MAX_LAYERS);
    PMGT_CHECK(kind >= PMGT_NCF_MLP && kind <= PMGT_NCF_NEUMF_PRE, -2, "%s: unknown model kind %d", who, kind);
    const int d = factor_num << (num_layers - 1);
    const bool gmf_only = kind == PMGT_NCF_GMF;
    PMGT_CHECK(gmf_only || d <= NCF_MAX_D, -2, "%s: d = factor_num * 2^(num_layers - 1) = %d above %d", who, d, NCF_MAX_D);
    if (int rc = pair_check_rows(who, user_num, item_num)) return rc;
    *s = NmShape{factor_num, gmf_only ? 0 : num_layers, d, kind != PMGT_NCF_MLP, !gmf_only, (!gmf_only && use_layer_norm) ? 1 : 0,
                 (!gmf_only && train_items) ? 1 : 0, user_num, item_num};
    return 0;
}

// the flat parameter layout: off[PMGT_NCF_MODEL_TENSORS] in floats (-1 = the kind trains no such tensor) -> the parameter count
static int64_t nm_layout(const NmShape& s, int64_t* off) {
    int64_t at = 0;
    for (int i = 0; i < PMGT_NCF_MODEL_TENSORS; ++i) off[i] = -1;
    if (s.mlp) off[0] = at, at += s.user_num * s.d;
    if (s.gmf) {
        off[1] = at, at += s.user_num * s.F;
        off[2] = at, at += s.item_num * s.F;
    }
    for (int l = 0; l < s.L; ++l) {
        const int64_t out = s.d >> l;
        off[3 + 4 * l] = at, at += out * 2 * out;
        off[4 + 4 * l] = at, at += out;
        if (s.ln) {
            off[5 + 4 * l] = at, at += out;
            off[6 + 4 * l] = at, at += out;
        }
    }
    off[NM_OFF_WP] = at, at += (s.gmf && s.mlp) ? 2 * s.F : s.F;
    off[NM_OFF_BP] = at, at += 1;
    if (s.table) {
        at = (at + 7) / 8 * 8;
        off[NM_OFF_TABLE] = at, at += s.item_num * s.d;
    }
    return at;
}

// the workspace of the kernels of this file in floats: per layer y, h, g, dz [n][d >> l] and stat [n][2]; dx [n][2 d]; gprod / ggu / ggi
// [n][F]; pz [n][2]; the two orders (int [n] each)
static int64_t nm_workspace_floats(const NmShape& s, int64_t n) {
    int64_t w = 0;
    for (int l = 0; l < s.L; ++l) w += 4 * n * (s.d >> l) + (2 * n + 3) / 4 * 4;
    if (s.L) w += 2 * n * s.d;
    w += 3 * n * s.F;
    w += (2 * n + 3) / 4 * 4;
    w += 2 * ((n + 3) / 4 * 4);
    return w;
}

static bool nm_delegated(const NmShape& s) { return s.mlp && !s.ln; }      // the head ncf_train.hip trains: its entries, its bits

}  // namespace pmgt

using namespace pmgt;

extern "C" {

int64_t pmgt_ncf_model_layout(int factor_num, int num_layers, int kind, int use_layer_norm, int train_items, int64_t user_num, int64_t item_num,
                              int64_t* offsets) {
    NmShape s;
    if (int rc = nm_shape(factor_num, num_layers, kind, use_layer_norm, train_items, user_num, item_num, "pmgt_ncf_model_layout", &s)) return rc;
    int64_t off[PMGT_NCF_MODEL_TENSORS];
    const int64_t count = nm_layout(s, off);
    if (offsets)
        for (int i = 0; i < PMGT_NCF_MODEL_TENSORS; ++i) offsets[i] = off[i];
    return count;
}

int64_t pmgt_ncf_model_workspace_bytes(int factor_num, int num_layers, int kind, int use_layer_norm, int train_items, int64_t n) {
    const char* who = "pmgt_ncf_model_workspace_bytes";
    NmShape s;
    if (int rc = nm_shape(factor_num, num_layers, kind, use_layer_norm, train_items, 1, 1, who, &s)) return rc;
    if (int rc = pair_check_n(who, n, PMGT_NCF_TRAIN_MAX_PAIRS)) return rc;
    if (nm_delegated(s)) {
        const int k = s.gmf ? PMGT_NCF_NEUMF_END : PMGT_NCF_MLP;
        return s.table ? pmgt_ncf_train_table_workspace_bytes(factor_num, num_layers, k, n) : pmgt_ncf_train_workspace_bytes(factor_num, num_layers, k, n);
    }
    return nm_workspace_floats(s, n) * (int64_t)sizeof(float);
}

int pmgt_ncf_model_train_grad(const pmgt_ncf_model* m, const int64_t* users, const int64_t* items, const float* labels, int64_t n, float* loss,
                              float* logits, const pmgt_ncf_dropout* drop, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "pmgt_ncf_model_train_grad";
    PMGT_CHECK(m != nullptr, -2, "%s: NULL model", who);
    NmShape s;
    if (int rc = nm_shape(m->factor_num, m->num_layers, m->kind, m->use_layer_norm, m->train_items, m->user_num, m->item_num, who, &s)) return rc;
    PMGT_CHECK(std::isfinite(m->layer_norm_eps) && m->layer_norm_eps >= 0.f, -2, "%s: layer_norm_eps = %g is not finite or negative", who,
               (double)m->layer_norm_eps);
    if (int rc = pair_check_n(who, n, PMGT_NCF_TRAIN_MAX_PAIRS)) return rc;
    PMGT_CHECK((!s.mlp || m->item_table) && m->params && m->grads && users && items && labels && loss && workspace, -2, "%s: NULL buffer", who);
    PMGT_CHECK(!s.table || m->table_grad, -2, "%s: NULL table_grad", who);
    const uintptr_t table_bits = s.mlp ? (uintptr_t)m->item_table | (s.table ? (uintptr_t)m->table_grad : 0) : 0;
    PMGT_CHECK(((table_bits | (uintptr_t)m->params | (uintptr_t)m->grads | (uintptr_t)workspace) & 15) == 0, -2,
               "%s: the item table, the parameters, the gradients (the table's included) and the workspace must be 16-byte aligned", who);
    if (int rc = pair_check_small(who, users, items, labels, loss, logits)) return rc;
    const int64_t need = pmgt_ncf_model_workspace_bytes(m->factor_num, m->num_layers, m->kind, m->use_layer_norm, m->train_items, n);
    PMGT_CHECK(workspace_bytes >= need, -2, "%s: workspace of %lld bytes below the %lld needed", who, (long long)workspace_bytes, (long long)need);
    NmDrop dr;
    bool drop_on;                                            // every p 0: the instantiations without dropout
    if (int rc = pair_check_ncf_dropout(who, drop, s.L, &dr, &drop_on)) return rc;
    if (nm_delegated(s)) {                                   // the layouts agree: the head part of nm_layout is pmgt_ncf_train_layout's
        const pmgt_ncf_train head = {s.F, s.L, s.gmf ? PMGT_NCF_NEUMF_END : PMGT_NCF_MLP, 0, s.user_num, s.item_num, m->item_table, m->params, m->grads};
        float* tg = s.table ? m->table_grad : nullptr;
        if (drop) return pmgt_ncf_train_grad_dropout(&head, users, items, labels, n, loss, logits, tg, &dr, workspace, workspace_bytes, stream);
        if (tg) return pmgt_ncf_train_grad_table(&head, users, items, labels, n, loss, logits, tg, workspace, workspace_bytes, stream);
        return pmgt_ncf_train_grad(&head, users, items, labels, n, loss, logits, workspace, workspace_bytes, stream);
    }
    int64_t off[PMGT_NCF_MODEL_TENSORS];
    nm_layout(s, off);
    const float* P = m->params;
    float* G = m->grads;
    float* ws = (float*)workspace;
    const int F = s.F, L = s.L, d = s.d;

    NmPairsArgs pa = {};
    NmGradsArgs ga = {};
    for (int l = 0; l < L; ++l) {
        const int out = d >> l;
        NmLayer& ly = pa.layer[l];
        ly.w = P + off[3 + 4 * l], ly.b = P + off[4 + 4 * l], ly.gamma = P + off[5 + 4 * l], ly.beta = P + off[6 + 4 * l];
        ly.out = out;
        ly.y = ws, ws += n * out;
        ly.h = ws, ws += n * out;
        ly.g = ws, ws += n * out;
        ly.dz = ws, ws += n * out;
        ly.stat = ws, ws += (2 * n + 3) / 4 * 4;
    }
    if (L) pa.dx = ws, ws += n * 2 * d;
    pa.gprod = ws, ws += n * F;
    pa.ggu = ws, ws += n * F;
    pa.ggi = ws, ws += n * F;
    pa.pz = ws, ws += (2 * n + 3) / 4 * 4;
    pa.order_u = (int*)ws, ws += (n + 3) / 4 * 4;
    pa.order_i = (int*)ws;
    pa.u_mlp = s.mlp ? P + off[0] : nullptr;
    pa.table = s.mlp ? m->item_table : nullptr;
    pa.gu = s.gmf ? P + off[1] : nullptr;
    pa.gi = s.gmf ? P + off[2] : nullptr;
    pa.wp = P + off[NM_OFF_WP];
    pa.bp = P + off[NM_OFF_BP];
    pa.users = users, pa.items = items, pa.labels = labels, pa.logits = logits;
    pa.zero_base = G;
    pa.zero_vec4 = (L ? off[3] : off[NM_OFF_WP]) / 4;        // the embedding tables come first; every size is a multiple of 8 floats
    pa.zero2_base = s.table ? m->table_grad : nullptr;
    pa.zero2_vec4 = s.table ? s.item_num * d / 4 : 0;
    pa.eps = m->layer_norm_eps;
    pa.n = (int)n, pa.d = d, pa.factor = F, pa.num_layers = L, pa.gmf = s.gmf;
    pa.tiles = (int)cdiv64(n, PAIR_TILE);
    pa.rank_blocks = (int)cdiv64(n, PAIR_THREADS);
    pa.zero_blocks = (int)std::min<int64_t>(PAIR_ZERO_BLOCKS, cdiv64(pa.zero_vec4 + pa.zero2_vec4, PAIR_THREADS));

    int first = 0;
    for (int l = 0; l < L; ++l) {
        const int out = d >> l;
        pair_add_task(ga.task, &ga.ntasks, &first, pa.layer[l].dz, out,
                      l == 0 ? PairSrc{pa.u_mlp, users, d, pa.table, items, d} : PairSrc{pa.layer[l - 1].h, nullptr, 2 * out, nullptr, nullptr, 0},
                      G + off[3 + 4 * l], G + off[4 + 4 * l], false);
    }
    const PairSrc feat = L ? PairSrc{pa.layer[L - 1].h, nullptr, F, nullptr, nullptr, 0} : PairSrc{pa.gprod, nullptr, F, nullptr, nullptr, 0};
    pair_add_task(ga.task, &ga.ntasks, &first, pa.pz, 2, (s.gmf && L) ? PairSrc{pa.gprod, nullptr, F, pa.layer[L - 1].h, nullptr, F} : feat,
                  G + off[NM_OFF_WP], G + off[NM_OFF_BP], true);
    ga.weight_blocks = first;
    int cfirst = 0;
    for (int l = 0; l < L; ++l) {
        NmJob& jb = ga.job[l];
        jb.g = pa.layer[l].g, jb.y = pa.layer[l].y, jb.stat = pa.layer[l].stat;
        jb.ggamma = G + off[5 + 4 * l], jb.gbeta = G + off[6 + 4 * l];
        jb.W = d >> l;
        jb.first = cfirst;
        cfirst += (jb.W + 63) / 64;
    }
    ga.njobs = L;
    ga.col_blocks = cfirst;
    ga.row_blocks = (int)cdiv64(n, PAIR_WAVES);
    ga.users = users, ga.items = items;
    ga.order_u = pa.order_u, ga.order_i = pa.order_i;
    ga.dx = pa.dx, ga.ggu = pa.ggu, ga.ggi = pa.ggi;
    ga.g_u_mlp = s.mlp ? G + off[0] : nullptr;
    ga.g_gu = s.gmf ? G + off[1] : nullptr;
    ga.g_gi = s.gmf ? G + off[2] : nullptr;
    ga.g_table = s.table ? m->table_grad : nullptr;
    ga.loss = loss;
    ga.n = (int)n, ga.d = d, ga.factor = F, ga.gmf = s.gmf, ga.mlp = s.mlp;

    hipStream_t st = (hipStream_t)stream;
    const int kinds = (s.gmf || s.table) ? 2 : 1;            // MLP over frozen items has no rows indexed by item
    const unsigned grid1 = (unsigned)(pa.tiles + 2 * pa.rank_blocks + pa.zero_blocks);
    if (drop_on) hipLaunchKernelGGL((ncf_model_pairs_kernel<true>), dim3(grid1), dim3(PAIR_THREADS), 0, st, pa, dr);
    else hipLaunchKernelGGL((ncf_model_pairs_kernel<false>), dim3(grid1), dim3(PAIR_THREADS), 0, st, pa, dr);
    PMGT_LAUNCH_OK();
    const unsigned grid2 = (unsigned)(ga.weight_blocks + ga.col_blocks + kinds * ga.row_blocks);
    if (drop_on && L && dr.p_emb > 0.f) hipLaunchKernelGGL((ncf_model_grads_kernel<true>), dim3(grid2), dim3(PAIR_THREADS), 0, st, ga, dr);
    else hipLaunchKernelGGL((ncf_model_grads_kernel<false>), dim3(grid2), dim3(PAIR_THREADS), 0, st, ga, dr);
    PMGT_LAUNCH_OK();
    return 0;
}

}  // extern "C"
