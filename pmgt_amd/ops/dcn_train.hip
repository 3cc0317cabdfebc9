// The Deep & Cross Network of the reference's click-through experiment (pmgt/dcn/models.py; pmgt_dcn_forward and pmgt_dcn_train_grad of
// include/pmgt_capi.h, where the formulae stand): logits, or loss, logits and the gradient of the mean BCE-with-logits loss with respect to
// every trained parameter, both embedding tables included, for n (user, item, label) pairs, in TWO launches.  Kept out of csrc/ for
// ncf_train.hip's reason: the measured step launches nothing of this.  The Linear layers and their gradients are the pair-major products of
// pair_train_tile.h, which also states the roles rank / zero / weight / rows and the chain policies: Chain::ONE without dropout,
// Chain::BLOCK in the DROP instantiations, no activation in the epilogue, one row source and no input mask.  Everything else is ROW WORK:
// one wave owns one pair's row (up to D = 512 floats, 8 a lane as two 16-byte pieces) and reduces over it with a shuffle butterfly.
//
// EVERYTHING IS PAIR-MAJOR in the caller's workspace: x0 [n][D], the deep net's y_l = W_l h_l + b_l, h_(l+1), g_l = d loss / d LN_l's
// output behind the ReLU and dy_l = d loss / d y_l, each [n][D >> (l + 1)]; the cross net's final x^(C) [n][D] and, with LayerNorm, G_c = d loss
// / d x^(c+1) [n][D] per layer; four statistics per pair and layer (cross: s_c, mean, rstd, ds_c; deep: -, mean, rstd, -).  The cross
// states x^(c) themselves are NOT stored: x^(c+1) = ((x0 s_c + x0) - mean) rstd gamma + beta is recomputed from x0 and the statistics by
// the same sequence of operations wherever it is needed (the file is compiled without contraction, so the bits agree).
//
// LAUNCH 1, dcn_pairs_kernel (the forward entry launches the tiles only, instantiated without the backward): the roles rank and zero (the
// gradient rows of the two embedding tables), and
//   tile   32 pairs a workgroup of 4 waves.  Gathers x0; deep forward: per layer the MFMA product then, per pair row, LayerNorm and ReLU;
//          cross forward per pair row, wave w taking pairs 8 w .. 8 w + 7: the dot with w_c, x0 s + x0, LayerNorm; the output layer, the
//          loss and dz.  Then back: per deep layer the row pass (ReLU mask, LayerNorm backward) and the MFMA data gradient, down to d x0's
//          deep part; per pair row the cross chain from layer C - 1 to 0, which adds its terms in that order, then d x^(0), then the deep
//          part.  A workgroup reads only what it wrote itself, behind a barrier.
// LAUNCH 2, dcn_grads_kernel: the roles weight (the output layer is the pseudo-layer against [x^(C) ; h_L]) and rows (the two halves of
// d x0), and
//   cols   64 columns a workgroup: gamma, beta and w_c gradients, wave a summing the pairs a, a + 4, .. in order, added as (w0 + w1) +
//          (w2 + w3).
//
// DROPOUT (pmgt_dcn_train_grad_dropout; the DROP instantiations, which alone read the second kernel argument): the model in training
// mode, every mask m = 0 or 1 / (1 - p) drawn by the counter-based RNG of csrc/common.h at (site, row = the pair, column = the feature):
//   x0 = m_e [user ; item]   x^(c+1) = LN_c(m_c (x0 s_c) + x0)   h_(l+1) = relu(LN_l(m_l (W_l h_l + b_l)))
// No mask is stored.  The gather stores the DROPPED x0 and the deep epilogue the DROPPED y_l, so everything downstream (the row passes,
// the weight tasks of launch 2) reads dropped operands as they are; m_c is drawn again wherever x^(c+1) is recomputed (the cross
// backward and the cols role, the same sequence (x0 s) m + x0); back: dy_l = m_l LNbwd(..) (without LayerNorm h > 0 already names the
// kept elements and the factor 1 / (1 - p_l) suffices), ds_c = sum_j g_j m_cj x0_j, d x0 += g (m_c s_c) + g, and the final d x0 is
// multiplied by m_e before the store.  A site with p = 0 draws nothing; launch 2 runs its DROP instantiation only when a p_cross is > 0.
// ARITHMETIC OF THE DROP INSTANTIATIONS of launch 1: the row reductions (s_c, the LayerNorm statistics and the sums of its backward, ds_c,
// the output layer's dots) add exact products in fp64 and round to fp32 once, for Chain::BLOCK's reason.  Statistics are stored and only
// READ by the second launch, so what it recomputes from them agrees as before.
#include "pair_train_tile.h"

#pragma clang fp contract(off)

namespace pmgt {

static constexpr int DC_PER_WAVE = PAIR_TILE / PAIR_WAVES, DC_MAX_DEEP = PMGT_DCN_MAX_DEEP, DC_MAX_CROSS = PMGT_DCN_MAX_CROSS;
static constexpr int DC_MAX_TASKS = DC_MAX_DEEP + 1, DC_MAX_JOBS = 2 * DC_MAX_DEEP + 3 * DC_MAX_CROSS, DC_MAX_E = 256;

struct DcDeep {
    const float *w, *b, *gamma, *beta;      // [out][in], [out], LayerNorm [out] (NULL without)
    float *y, *h, *g, *dy, *st;             // workspace [n][out] x 4 (g: LayerNorm only), statistics [n][4]
    int out, in;
};

struct DcCross {
    const float *w, *gamma, *beta;          // [D] each
    float* G;                               // workspace [n][D]: d loss / d x^(c+1) (LayerNorm only)
};

struct DcPairsArgs {
    DcDeep deep[DC_MAX_DEEP];
    DcCross cross[DC_MAX_CROSS];
    const float *users_t, *items_t, *wo, *bo;
    const int64_t *users, *items;
    const float* labels;
    float *x0, *xC, *dx0, *cst, *pz;        // workspace: [n][D] x 3, [n][C][4], [n][2] = (dz, loss of the pair)
    int *order_u, *order_i;
    float* logits;
    float* zero_base;
    int64_t zero_vec4;
    float eps;
    int n, E, D, F, L, C, tiles, rank_blocks, zero_blocks;
};

enum { DC_JOB_SUM = 0, DC_JOB_DEEP_GAMMA = 1, DC_JOB_CROSS_GAMMA = 2, DC_JOB_CROSS_W = 3 };

struct DcJob {
    const float* a;          // SUM / GAMMA: [n][W]; CROSS_W: ds_c of pair p at a[p * stride]
    const float* x;          // DEEP_GAMMA: y_l; CROSS_*: x0
    const float* st;         // the statistics of pair p at st[p * stride + {0: s, 1: mean, 2: rstd}]; CROSS_W: those of layer c - 1, NULL for c = 0
    const float *gamma, *beta;      // CROSS_W with LayerNorm: of layer c - 1
    float* out;
    int W, kind, first, stride;
};

struct DcGradsArgs {
    PairTask task[DC_MAX_TASKS];
    DcJob job[DC_MAX_JOBS];
    const int64_t *users, *items;
    const int *order_u, *order_i;
    const float* dx0;
    float *g_users, *g_items, *loss;
    int n, E, ntasks, njobs, weight_blocks, col_blocks, row_blocks;
};

// the second kernel argument; only the DROP instantiations read it
struct DcDrop {
    pmgt_dcn_dropout d;
    signed char job_cross[DC_MAX_JOBS];      // launch 2, per cols job: the cross layer whose mask its recomputation draws again, -1: none
};

// ---- a row of W <= 512 floats (W a multiple of 8) on a wave: lane holds the pieces lane and lane + 64, elements k = 4 j + e ----------
struct DcRow {
    int col[2];
    bool ok[2];
};
__device__ __forceinline__ DcRow dc_row(int W, int lane) {
    DcRow r;
#pragma unroll
    for (int j = 0; j < 2; ++j) r.col[j] = 4 * (lane + 64 * j), r.ok[j] = r.col[j] < W;
    return r;
}
__device__ __forceinline__ void dc_row_ld(float (&e)[8], const float* p, const DcRow& r) {      // elements outside the row are 0
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const float4 v = pair_ld4(p + r.col[j], r.ok[j]);
        e[4 * j] = v.x, e[4 * j + 1] = v.y, e[4 * j + 2] = v.z, e[4 * j + 3] = v.w;
    }
}
__device__ __forceinline__ void dc_row_st(float* p, const float (&e)[8], const DcRow& r) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
        if (r.ok[j]) *reinterpret_cast<float4*>(p + r.col[j]) = make_float4(e[4 * j], e[4 * j + 1], e[4 * j + 2], e[4 * j + 3]);
}
__device__ __forceinline__ double dc_wave_sum64(double x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
// HI (the DROP instantiations): the products are exact and the sum runs in fp64, rounded to fp32 once -- a reduction over a row then
// carries half an ulp instead of the in-order sum's few; the instantiations without dropout keep their arithmetic and their bits
template <bool HI = false>
__device__ __forceinline__ float dc_row_dot(const float (&a)[8], const float (&b)[8]) {
    if constexpr (HI) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) s += (double)a[k] * (double)b[k];
        return (float)dc_wave_sum64(s);
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += a[k] * b[k];
    return pair_wave_sum(s);
}
template <bool HI = false>
__device__ __forceinline__ float dc_row_sum(const float (&a)[8]) {
    if constexpr (HI) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) s += (double)a[k];
        return (float)dc_wave_sum64(s);
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) s += a[k];
    return pair_wave_sum(s);
}
// u -> (u - mean) rstd, the statistics out
template <bool HI = false>
__device__ __forceinline__ void dc_ln_stats(float (&u)[8], const DcRow& r, int W, float eps, float& mean, float& rstd) {
    mean = dc_row_sum<HI>(u) / (float)W;
#pragma unroll
    for (int k = 0; k < 8; ++k) u[k] = r.ok[k >> 2] ? u[k] - mean : 0.f;
    rstd = 1.f / sqrtf(dc_row_dot<HI>(u, u) / (float)W + eps);
#pragma unroll
    for (int k = 0; k < 8; ++k) u[k] = u[k] * rstd;
}
// u -> (u - mean) rstd with given statistics (what dc_ln_stats left, bit for bit)
__device__ __forceinline__ void dc_ln_xhat(float (&u)[8], const DcRow& r, float mean, float rstd) {
#pragma unroll
    for (int k = 0; k < 8; ++k) u[k] = (r.ok[k >> 2] ? u[k] - mean : 0.f) * rstd;
}
__device__ __forceinline__ void dc_affine(float (&x)[8], const float* gamma, const float* beta, const DcRow& r) {
    float g[8], b[8];
    dc_row_ld(g, gamma, r);
    dc_row_ld(b, beta, r);
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = x[k] * g[k] + b[k];
}
// g = d loss / d LN output -> d loss / d LN input
template <bool HI = false>
__device__ __forceinline__ void dc_ln_bwd(float (&g)[8], const float (&xhat)[8], const float* gamma, const DcRow& r, int W, float rstd) {
    float gm[8];
    dc_row_ld(gm, gamma, r);
#pragma unroll
    for (int k = 0; k < 8; ++k) g[k] = g[k] * gm[k];
    const float m1 = dc_row_sum<HI>(g) / (float)W, m2 = dc_row_dot<HI>(g, xhat) / (float)W;
#pragma unroll
    for (int k = 0; k < 8; ++k) g[k] = r.ok[k >> 2] ? rstd * ((g[k] - m1) - xhat[k] * m2) : 0.f;
}
// the cross layer's pre-LayerNorm value from x0: x0 s + x0
__device__ __forceinline__ void dc_cross_u(float (&u)[8], const float (&x0)[8], float s) {
#pragma unroll
    for (int k = 0; k < 8; ++k) u[k] = x0[k] * s + x0[k];
}

// ---- dropout (the DROP instantiations only) ---------------------------------------------------------------------------------------------
// the mask of a site on the lane's 8 elements of row `pair`: the pieces lane and lane + 64 are the column groups lane and lane + 64
__device__ __forceinline__ void dc_row_mask(float (&m)[8], const DropKey& k, int pair, int lane) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        float mk[4];
        drop_mul4(k, (uint32_t)pair, (uint32_t)(lane + 64 * j), mk);
#pragma unroll
        for (int e = 0; e < 4; ++e) m[4 * j + e] = mk[e];
    }
}
// the cross layer's pre-LayerNorm value under the layer's mask: (x0 s) m + x0
__device__ __forceinline__ void dc_cross_u_drop(float (&u)[8], const float (&x0)[8], float s, const float (&m)[8]) {
#pragma unroll
    for (int k = 0; k < 8; ++k) u[k] = (x0[k] * s) * m[k] + x0[k];
}

// TRAIN: the gradient entry (the forward entry is the same forward code without the stores and the phases only the backward needs)
// LN: use_layer_norm
// DROP: dropout is on at one site or more (without it the kernel's instructions are those it had: `dr` is not read)
template <bool TRAIN, bool LN, bool DROP>
__global__ __launch_bounds__(PAIR_THREADS) void dcn_pairs_kernel(DcPairsArgs a, DcDrop dr) {
    __shared__ float s_dl[PAIR_TILE];
    __shared__ int64_t s_ids[PAIR_THREADS];
    constexpr Chain DC_CHAIN = DROP ? Chain::BLOCK : Chain::ONE;
    const int tid = threadIdx.x, lane = tid & 63, wave = pair_wave_index(), n = a.n;
    const int bid = blockIdx.x;
    if constexpr (TRAIN) {
        if (bid >= a.tiles + 2 * a.rank_blocks) {            // ---- zero: the gradients of the two embedding tables, whole
            pair_zero<false>(bid - a.tiles - 2 * a.rank_blocks, a.zero_blocks, a.zero_base, a.zero_vec4, nullptr, 0, tid);
            return;
        }
        if (bid >= a.tiles) {                                // ---- rank: the stable order by id, counted
            pair_rank(bid - a.tiles, a.rank_blocks, n, a.users, a.items, a.order_u, a.order_i, s_ids, tid);
            return;
        }
    }
    // ---- tile: 32 pairs
    const int D = a.D, E = a.E, L = a.L, C = a.C;
    const int mpair = bid * PAIR_TILE + (lane & 31);           // the lane's pair in the MFMA phases
    const bool mvalid = mpair < n;
    const DcRow rD = dc_row(D, lane);
    DropKey kemb = pair_drop_off();
    if constexpr (DROP) kemb = make_drop_key(DropCfg{dr.d.rng, dr.d.p_emb, DCN_SITE_EMB});
    // x0 = [users_t[u] ; items_t[i]]: a piece lies in one half (E is a multiple of 4)
    for (int i = 0; i < DC_PER_WAVE; ++i) {
        const int pair = bid * PAIR_TILE + wave * DC_PER_WAVE + i;
        if (pair >= n) break;                                // (uniform per wave)
        const float* urow = a.users_t + a.users[pair] * E;
        const float* irow = a.items_t + a.items[pair] * E;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            if (rD.ok[j]) {
                const int c = rD.col[j];
                if constexpr (DROP) {                        // the DROPPED x0 is stored: everything downstream reads it
                    float4 v = *reinterpret_cast<const float4*>(c < E ? urow + c : irow + (c - E));
                    if (kemb.on) {
                        float mk[4];
                        drop_mul4(kemb, (uint32_t)pair, (uint32_t)(c >> 2), mk);
                        v.x *= mk[0], v.y *= mk[1], v.z *= mk[2], v.w *= mk[3];
                    }
                    *reinterpret_cast<float4*>(a.x0 + (int64_t)pair * D + c) = v;
                } else {
                    *reinterpret_cast<float4*>(a.x0 + (int64_t)pair * D + c) = *reinterpret_cast<const float4*>(c < E ? urow + c : irow + (c - E));
                }
            }
    }
    __syncthreads();
    // deep forward
    for (int l = 0; l < L; ++l) {
        const DcDeep& dl = a.deep[l];
        const float* xin = l == 0 ? a.x0 : a.deep[l - 1].h;
        DropKey kdeep = pair_drop_off();                       // DROP: the stored y_l is the dropped one, and the row pass normalises that
        if constexpr (DROP) kdeep = make_drop_key(DropCfg{dr.d.rng, dr.d.p_deep[l], DCN_SITE_DEEP + (uint32_t)l});
        pair_linear<DC_CHAIN, false, DROP>(dl.w, dl.b, dl.out, dl.in, xin + (int64_t)mpair * dl.in, dl.in, nullptr, mvalid,
                                           dl.y + (int64_t)mpair * dl.out, wave, lane, pair_drop_off(), kdeep, mpair);
        __syncthreads();
        const DcRow r = dc_row(dl.out, lane);
        for (int i = 0; i < DC_PER_WAVE; ++i) {
            const int pair = bid * PAIR_TILE + wave * DC_PER_WAVE + i;
            if (pair >= n) break;
            float v[8];
            dc_row_ld(v, dl.y + (int64_t)pair * dl.out, r);
            if constexpr (LN) {
                float mean, rstd;
                dc_ln_stats<DROP>(v, r, dl.out, a.eps, mean, rstd);
                dc_affine(v, dl.gamma, dl.beta, r);
                if constexpr (TRAIN) {
                    if (lane == 0) dl.st[(int64_t)pair * 4 + 1] = mean, dl.st[(int64_t)pair * 4 + 2] = rstd;
                }
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = relu_keep_nan(v[k]);
            dc_row_st(dl.h + (int64_t)pair * dl.out, v, r);
        }
        __syncthreads();
    }
    // cross forward, the output layer, the loss
    const int HW = a.deep[L - 1].out;                        // 2 F
    const DcRow rH = dc_row(HW, lane);
    for (int i = 0; i < DC_PER_WAVE; ++i) {
        const int pl = wave * DC_PER_WAVE + i, pair = bid * PAIR_TILE + pl;
        if (pair >= n) {
            if (TRAIN && lane == 0) s_dl[pl] = 0.f;
            continue;
        }
        float e0[8], x[8], w[8];
        dc_row_ld(e0, a.x0 + (int64_t)pair * D, rD);
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] = e0[k];
        for (int c = 0; c < C; ++c) {
            dc_row_ld(w, a.cross[c].w, rD);
            const float s = dc_row_dot<DROP>(x, w);
            if constexpr (DROP) {
                const DropKey kc = make_drop_key(DropCfg{dr.d.rng, dr.d.p_cross[c], DCN_SITE_CROSS + (uint32_t)c});
                if (kc.on) {
                    float mk[8];
                    dc_row_mask(mk, kc, pair, lane);
                    dc_cross_u_drop(x, e0, s, mk);
                } else {
                    dc_cross_u(x, e0, s);
                }
            } else {
                dc_cross_u(x, e0, s);
            }
            float mean = 0.f, rstd = 0.f;
            if constexpr (LN) {
                dc_ln_stats<DROP>(x, rD, D, a.eps, mean, rstd);
                dc_affine(x, a.cross[c].gamma, a.cross[c].beta, rD);
            }
            if constexpr (TRAIN) {
                if (lane == 0) {
                    float* st = a.cst + ((int64_t)pair * C + c) * 4;
                    st[0] = s, st[1] = mean, st[2] = rstd;
                }
            }
        }
        if constexpr (TRAIN) dc_row_st(a.xC + (int64_t)pair * D, x, rD);
        dc_row_ld(w, a.wo, rD);
        const float zc = dc_row_dot<DROP>(x, w);
        float hrow[8];
        dc_row_ld(hrow, a.deep[L - 1].h + (int64_t)pair * HW, rH);
        dc_row_ld(w, a.wo + D, rH);
        const float z = (zc + dc_row_dot<DROP>(hrow, w)) + a.bo[0];
        if (lane == 0) {
            if (a.logits) a.logits[pair] = z;
            if constexpr (TRAIN) {
                float dz, loss;
                pair_bce<false>(z, a.labels[pair], n, dz, loss);
                a.pz[(int64_t)pair * 2] = dz;
                a.pz[(int64_t)pair * 2 + 1] = loss;
                s_dl[pl] = dz;
            }
        }
    }
    if constexpr (!TRAIN) return;
    __syncthreads();
    // deep backward
    for (int l = L - 1; l >= 0; --l) {
        const DcDeep& dl = a.deep[l];
        const DcRow r = dc_row(dl.out, lane);
        DropKey kdeep = pair_drop_off();
        if constexpr (DROP) kdeep = make_drop_key(DropCfg{dr.d.rng, dr.d.p_deep[l], DCN_SITE_DEEP + (uint32_t)l});
        for (int i = 0; i < DC_PER_WAVE; ++i) {
            const int pl = wave * DC_PER_WAVE + i, pair = bid * PAIR_TILE + pl;
            if (pair >= n) break;
            float g[8], hv[8];
            if (l == L - 1) {
                dc_row_ld(g, a.wo + D, r);
                const float dz = s_dl[pl];
#pragma unroll
                for (int k = 0; k < 8; ++k) g[k] = dz * g[k];
            } else {
                dc_row_ld(g, dl.dy + (int64_t)pair * dl.out, r);      // W_(l+1)^T dy_(l+1), left here by the data gradient below
            }
            dc_row_ld(hv, dl.h + (int64_t)pair * dl.out, r);
#pragma unroll
            for (int k = 0; k < 8; ++k) g[k] = hv[k] > 0.f ? g[k] : 0.f;
            if constexpr (LN) {
                dc_row_st(dl.g + (int64_t)pair * dl.out, g, r);
                const float mean = dl.st[(int64_t)pair * 4 + 1], rstd = dl.st[(int64_t)pair * 4 + 2];
                dc_row_ld(hv, dl.y + (int64_t)pair * dl.out, r);
                dc_ln_xhat(hv, r, mean, rstd);
                dc_ln_bwd<DROP>(g, hv, dl.gamma, r, dl.out, rstd);
                if constexpr (DROP) {                        // dy_l = m_l LNbwd(..): the mask drawn again
                    if (kdeep.on) {
                        float mk[8];
                        dc_row_mask(mk, kdeep, pair, lane);
#pragma unroll
                        for (int k = 0; k < 8; ++k) g[k] = g[k] * mk[k];
                    }
                }
            } else if constexpr (DROP) {                     // h > 0 names the kept elements: the factor 1 / (1 - p_l) suffices
#pragma unroll
                for (int k = 0; k < 8; ++k) g[k] = g[k] * kdeep.scale;
            }
            dc_row_st(dl.dy + (int64_t)pair * dl.out, g, r);
        }
        __syncthreads();
        float* dst = l == 0 ? a.dx0 : a.deep[l - 1].dy;
        pair_linear_bwd<DC_CHAIN, DROP>(dl.w, dl.out, dl.in, dl.in, dl.dy + (int64_t)mpair * dl.out, nullptr, mvalid, dst + (int64_t)mpair * dl.in,
                                        wave, lane, 1.f, pair_drop_off(), mpair);
        __syncthreads();
    }
    // cross backward and d x0
    for (int i = 0; i < DC_PER_WAVE; ++i) {
        const int pl = wave * DC_PER_WAVE + i, pair = bid * PAIR_TILE + pl;
        if (pair >= n) break;
        float e0[8], g[8], acc[8], t[8];
        dc_row_ld(e0, a.x0 + (int64_t)pair * D, rD);
        dc_row_ld(g, a.wo, rD);
        const float dz = s_dl[pl];
#pragma unroll
        for (int k = 0; k < 8; ++k) g[k] = dz * g[k], acc[k] = 0.f;
        for (int c = C - 1; c >= 0; --c) {
            float* st = a.cst + ((int64_t)pair * C + c) * 4;
            const float s = st[0];
            float ds;
            if constexpr (DROP) {
                const DropKey kc = make_drop_key(DropCfg{dr.d.rng, dr.d.p_cross[c], DCN_SITE_CROSS + (uint32_t)c});
                float mk[8];
                if (kc.on) {
                    dc_row_mask(mk, kc, pair, lane);
                } else {
#pragma unroll
                    for (int k = 0; k < 8; ++k) mk[k] = 1.f;
                }
                if constexpr (LN) {
                    dc_row_st(a.cross[c].G + (int64_t)pair * D, g, rD);
                    const float mean = st[1], rstd = st[2];
                    if (kc.on) dc_cross_u_drop(t, e0, s, mk);      // the forward's sequence of operations: the same bits
                    else dc_cross_u(t, e0, s);
                    dc_ln_xhat(t, rD, mean, rstd);
                    dc_ln_bwd<true>(g, t, a.cross[c].gamma, rD, D, rstd);
                }
#pragma unroll
                for (int k = 0; k < 8; ++k) t[k] = g[k] * mk[k];      // d loss / d (x0 s_c)
                ds = dc_row_dot<true>(t, e0);
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[k] = acc[k] + (t[k] * s + g[k]);
            } else {
                if constexpr (LN) {
                    dc_row_st(a.cross[c].G + (int64_t)pair * D, g, rD);
                    const float mean = st[1], rstd = st[2];
                    dc_cross_u(t, e0, s);
                    dc_ln_xhat(t, rD, mean, rstd);
                    dc_ln_bwd(g, t, a.cross[c].gamma, rD, D, rstd);
                }
                ds = dc_row_dot(g, e0);
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[k] = acc[k] + (g[k] * s + g[k]);
            }
            if (lane == 0) st[3] = ds;
            dc_row_ld(t, a.cross[c].w, rD);
#pragma unroll
            for (int k = 0; k < 8; ++k) g[k] = ds * t[k];
        }
        dc_row_ld(t, a.dx0 + (int64_t)pair * D, rD);         // the deep net's part
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = (acc[k] + g[k]) + t[k];
        if constexpr (DROP) {                                // d [user ; item] = m_e d x0: the rows role adds what is stored
            if (kemb.on) {
                dc_row_mask(t, kemb, pair, lane);
#pragma unroll
                for (int k = 0; k < 8; ++k) acc[k] = acc[k] * t[k];
            }
        }
        dc_row_st(a.dx0 + (int64_t)pair * D, acc, rD);
    }
}

// DROP: a cross layer's mask is on: the cols role draws it again where it recomputes x^(c) / xhat (the weight and rows roles read stored,
// already dropped operands and need nothing)
template <bool LN, bool DROP>
__global__ __launch_bounds__(PAIR_THREADS) void dcn_grads_kernel(DcGradsArgs a, DcDrop dr) {
    __shared__ float s_acc[PAIR_WAVES][16][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = pair_wave_index(), n = a.n;
    int bid = blockIdx.x;
    if (bid >= a.weight_blocks + a.col_blocks) {             // ---- rows: segment sums of d x0's halves in pair order
        const PairRun r = pair_run(bid - a.weight_blocks - a.col_blocks, a.row_blocks, wave, n, a.users, a.items, a.order_u, a.order_i);
        if (!r.start) return;
        const int E = a.E;
        const float* src = a.dx0 + (r.kind ? E : 0);
        float* dst = (r.kind ? a.g_items : a.g_users) + r.id * E;
        for (int c = lane; c < E; c += 64) dst[c] = pair_run_sum(r, n, src, 2 * E, c);
        return;
    }
    if (bid >= a.weight_blocks) {                            // ---- cols: sums over the pairs of 64 columns
        bid -= a.weight_blocks;
        int ji = 0;
        for (int i = 1; i < a.njobs; ++i)
            if (bid >= a.job[i].first) ji = i;
        const DcJob& jb = a.job[ji];
        const int col = (bid - jb.first) * 64 + lane, W = jb.W;
        const bool ok = col < W;
        float gam = 0.f, bet = 0.f;
        if (LN && jb.kind == DC_JOB_CROSS_W && jb.st && ok) gam = jb.gamma[col], bet = jb.beta[col];
        DropKey kc = pair_drop_off();
        if constexpr (DROP) {
            const int mc = dr.job_cross[ji];
            if (mc >= 0) kc = make_drop_key(DropCfg{dr.d.rng, dr.d.p_cross[mc], DCN_SITE_CROSS + (uint32_t)mc});
        }
        float sum = 0.f;
        for (int p = wave; p < n; p += PAIR_WAVES) {
            if (!ok) break;
            const int64_t at = (int64_t)p * W + col;
            float v;
            if (jb.kind == DC_JOB_SUM) {
                v = jb.a[at];
            } else if (jb.kind == DC_JOB_DEEP_GAMMA) {
                const float* st = jb.st + (int64_t)p * jb.stride;
                v = jb.a[at] * ((jb.x[at] - st[1]) * st[2]);
            } else if (jb.kind == DC_JOB_CROSS_GAMMA) {
                const float* st = jb.st + (int64_t)p * jb.stride;
                const float x0 = jb.x[at];
                if (DROP && kc.on) v = jb.a[at] * ((((x0 * st[0]) * drop_mul1(kc, (uint32_t)p, (uint32_t)col) + x0) - st[1]) * st[2]);
                else v = jb.a[at] * (((x0 * st[0] + x0) - st[1]) * st[2]);
            } else {
                float x = jb.x[at];
                if (jb.st) {                                 // x^(c) from x0 and the statistics of layer c - 1
                    const float* st = jb.st + (int64_t)p * jb.stride;
                    if (DROP && kc.on) x = (x * st[0]) * drop_mul1(kc, (uint32_t)p, (uint32_t)col) + x;
                    else x = x * st[0] + x;
                    if constexpr (LN) x = ((x - st[1]) * st[2]) * gam + bet;
                }
                v = jb.a[(int64_t)p * jb.stride] * x;
            }
            sum += v;
        }
        s_acc[wave][0][lane] = sum;
        __syncthreads();
        if (wave == 0 && ok) jb.out[col] = (s_acc[0][0][lane] + s_acc[1][0][lane]) + (s_acc[2][0][lane] + s_acc[3][0][lane]);
        return;
    }
    // ---- weight: one 32 x 32 block of dW = dy^T x, the pairs in order
    pair_weight_block<false, false>(a.task, a.ntasks, bid, n, a.loss, DropCfg{}, s_acc, tid, lane, wave);
}

struct DcShape {
    int F, L, C, ln, E, D;
    int64_t user_num, item_num;
};

static int dc_shape(int F, int L, int C, int ln, int64_t user_num, int64_t item_num, const char* who, DcShape* s) {
    PMGT_CHECK(F == 8 || F == 16 || F == 32 || F == 64, -2, "%s: factor_num = %d, covered: 8, 16, 32, 64", who, F);
    PMGT_CHECK(L >= 1 && L <= DC_MAX_DEEP, -2, "%s: deep_layers = %d outside [1, %d]", who, L, DC_MAX_DEEP);
    PMGT_CHECK((F << L) <= DC_MAX_E, -2, "%s: E = factor_num * 2^deep_layers = %d above %d", who, F << L, DC_MAX_E);
    PMGT_CHECK(C >= 1 && C <= DC_MAX_CROSS, -2, "%s: cross_layers = %d outside [1, %d]", who, C, DC_MAX_CROSS);
    PMGT_CHECK(ln == 0 || ln == 1, -2, "%s: use_layer_norm = %d, expected 0 or 1", who, ln);
    if (int rc = pair_check_rows(who, user_num, item_num)) return rc;
    *s = DcShape{F, L, C, ln, F << L, 2 * (F << L), user_num, item_num};
    return 0;
}

// the flat parameter layout: off[PMGT_DCN_TENSORS] in floats (-1 = the model has no such tensor) -> the parameter count
static int64_t dc_layout(const DcShape& s, int64_t* off) {
    int64_t at = 0;
    for (int i = 0; i < PMGT_DCN_TENSORS; ++i) off[i] = -1;
    off[0] = at, at += s.user_num * s.E;
    off[1] = at, at += s.item_num * s.E;
    for (int l = 0; l < s.L; ++l) {
        const int64_t out = s.D >> (l + 1), in = s.D >> l;
        off[2 + 4 * l] = at, at += out * in;
        off[3 + 4 * l] = at, at += out;
        if (s.ln) {
            off[4 + 4 * l] = at, at += out;
            off[5 + 4 * l] = at, at += out;
        }
    }
    for (int c = 0; c < s.C; ++c)
        for (int j = 0; j < (s.ln ? 3 : 1); ++j) off[18 + 3 * c + j] = at, at += s.D;
    off[36] = at, at += s.D + 2 * s.F;
    off[37] = at, at += 1;
    return at;
}

// the workspace in floats: x0, x^(C), d x0 [n][D]; G_c [n][D] per cross layer (LayerNorm); the cross statistics [n][C][4]; per deep
// layer y, h, dy (LayerNorm: and g) [n][out] and the statistics [n][4]; pz [n][2]; the two orders (int [n] each)
static int64_t dc_workspace_floats(const DcShape& s, int64_t n) {
    int64_t w = 3 * n * s.D + (s.ln ? s.C * n * s.D : 0) + n * s.C * 4;
    for (int l = 0; l < s.L; ++l) w += (s.ln ? 4 : 3) * n * (s.D >> (l + 1)) + n * 4;
    w += (2 * n + 3) / 4 * 4;
    w += 2 * ((n + 3) / 4 * 4);
    return w;
}

// every entry; drop: NULL or the dropout of the call (the gradient entry only)
static int dc_run(const char* who, bool train, const pmgt_dcn_head* head, const int64_t* users, const int64_t* items, const float* labels,
                  int64_t n, float* loss, float* logits, const pmgt_dcn_dropout* drop, void* workspace, int64_t workspace_bytes, void* stream) {
    PMGT_CHECK(head != nullptr, -2, "%s: NULL head", who);
    DcShape s;
    if (int rc = dc_shape(head->factor_num, head->deep_layers, head->cross_layers, head->use_layer_norm, head->user_num, head->item_num, who, &s))
        return rc;
    if (int rc = pair_check_n(who, n, PMGT_DCN_MAX_PAIRS)) return rc;
    PMGT_CHECK(head->layer_norm_eps >= 0.f, -2, "%s: layer_norm_eps = %g is NaN or negative", who, (double)head->layer_norm_eps);      // (a NaN fails)
    PMGT_CHECK(head->params && users && items && workspace, -2, "%s: NULL buffer", who);
    PMGT_CHECK(train ? (head->grads && labels && loss) : logits != nullptr, -2, "%s: NULL buffer", who);
    PMGT_CHECK((((uintptr_t)head->params | (uintptr_t)(train ? head->grads : nullptr) | (uintptr_t)workspace) & 15) == 0, -2,
               "%s: the parameters, the gradients and the workspace must be 16-byte aligned", who);
    if (int rc = pair_check_small(who, users, items, labels, loss, logits)) return rc;
    const int64_t need = dc_workspace_floats(s, n) * (int64_t)sizeof(float);
    PMGT_CHECK(workspace_bytes >= need, -2, "%s: workspace of %lld bytes below the %lld needed", who, (long long)workspace_bytes, (long long)need);
    DcDrop dr = {};
    bool drop_on = false, cross_on = false;                  // every p 0: the instantiations without dropout
    if (drop) {
        dr.d.rng = drop->rng, dr.d.p_emb = drop->p_emb;
        if (int rc = pair_check_p(who, "p_emb", -1, dr.d.p_emb, &drop_on)) return rc;
        for (int l = 0; l < s.L; ++l) {
            dr.d.p_deep[l] = drop->p_deep[l];
            if (int rc = pair_check_p(who, "p_deep", l, dr.d.p_deep[l], &drop_on)) return rc;
        }
        for (int c = 0; c < s.C; ++c) {
            dr.d.p_cross[c] = drop->p_cross[c];
            if (int rc = pair_check_p(who, "p_cross", c, dr.d.p_cross[c], &cross_on)) return rc;
        }
        drop_on = drop_on || cross_on;
        if (int rc = pair_check_rng(who, drop_on, dr.d.rng)) return rc;
    }
    int64_t off[PMGT_DCN_TENSORS];
    dc_layout(s, off);
    const float* P = head->params;
    float* G = train ? head->grads : nullptr;
    float* ws = (float*)workspace;
    const int D = s.D, L = s.L, C = s.C;

    DcPairsArgs pa = {};
    pa.x0 = ws, ws += n * D;
    pa.xC = ws, ws += n * D;
    pa.dx0 = ws, ws += n * D;
    for (int c = 0; c < C; ++c) {
        pa.cross[c].w = P + off[18 + 3 * c];
        pa.cross[c].gamma = s.ln ? P + off[19 + 3 * c] : nullptr;
        pa.cross[c].beta = s.ln ? P + off[20 + 3 * c] : nullptr;
        if (s.ln) pa.cross[c].G = ws, ws += n * D;
    }
    pa.cst = ws, ws += n * C * 4;
    for (int l = 0; l < L; ++l) {
        DcDeep& d = pa.deep[l];
        d.out = D >> (l + 1), d.in = D >> l;
        d.w = P + off[2 + 4 * l];
        d.b = P + off[3 + 4 * l];
        d.gamma = s.ln ? P + off[4 + 4 * l] : nullptr;
        d.beta = s.ln ? P + off[5 + 4 * l] : nullptr;
        d.y = ws, ws += n * d.out;
        d.h = ws, ws += n * d.out;
        d.dy = ws, ws += n * d.out;
        if (s.ln) d.g = ws, ws += n * d.out;
        d.st = ws, ws += n * 4;
    }
    pa.pz = ws, ws += (2 * n + 3) / 4 * 4;
    pa.order_u = (int*)ws, ws += (n + 3) / 4 * 4;
    pa.order_i = (int*)ws;
    pa.users_t = P + off[0], pa.items_t = P + off[1];
    pa.wo = P + off[36], pa.bo = P + off[37];
    pa.users = users, pa.items = items, pa.labels = labels, pa.logits = logits;
    pa.zero_base = G;
    pa.zero_vec4 = off[2] / 4;                               // the two tables come first; E is a multiple of 8
    pa.eps = head->layer_norm_eps;
    pa.n = (int)n, pa.E = s.E, pa.D = D, pa.F = s.F, pa.L = L, pa.C = C;
    pa.tiles = (int)cdiv64(n, PAIR_TILE);
    pa.rank_blocks = (int)cdiv64(n, PAIR_THREADS);
    pa.zero_blocks = (int)std::min<int64_t>(PAIR_ZERO_BLOCKS, cdiv64(pa.zero_vec4, PAIR_THREADS));
    hipStream_t st = (hipStream_t)stream;
    if (!train) {
        if (s.ln) hipLaunchKernelGGL((dcn_pairs_kernel<false, true, false>), dim3((unsigned)pa.tiles), dim3(PAIR_THREADS), 0, st, pa, dr);
        else hipLaunchKernelGGL((dcn_pairs_kernel<false, false, false>), dim3((unsigned)pa.tiles), dim3(PAIR_THREADS), 0, st, pa, dr);
        PMGT_LAUNCH_OK();
        return 0;
    }

    DcGradsArgs ga = {};
    int first = 0;
    for (int l = 0; l < L; ++l)
        pair_add_task(ga.task, &ga.ntasks, &first, pa.deep[l].dy, pa.deep[l].out,
                      PairSrc{l == 0 ? pa.x0 : pa.deep[l - 1].h, nullptr, pa.deep[l].in, nullptr, nullptr, 0}, G + off[2 + 4 * l], G + off[3 + 4 * l], false);
    pair_add_task(ga.task, &ga.ntasks, &first, pa.pz, 2, PairSrc{pa.xC, nullptr, D, pa.deep[L - 1].h, nullptr, 2 * s.F}, G + off[36], G + off[37], true);
    ga.weight_blocks = first;
    int nj = 0, cfirst = 0;
    auto add_job = [&](int kind, const float* a, const float* x, const float* stp, int stride, const float* gm, const float* bt, float* out, int W,
                       int mask_cross) {                     // mask_cross: the cross layer whose statistics the job recomputes from, -1: none
        dr.job_cross[nj] = (signed char)mask_cross;
        DcJob& j = ga.job[nj++];
        j.kind = kind, j.a = a, j.x = x, j.st = stp, j.stride = stride, j.gamma = gm, j.beta = bt, j.out = out, j.W = W, j.first = cfirst;
        cfirst += (W + 63) / 64;
    };
    for (int l = 0; l < L && s.ln; ++l) {
        const DcDeep& d = pa.deep[l];
        add_job(DC_JOB_DEEP_GAMMA, d.g, d.y, d.st, 4, nullptr, nullptr, G + off[4 + 4 * l], d.out, -1);
        add_job(DC_JOB_SUM, d.g, nullptr, nullptr, 0, nullptr, nullptr, G + off[5 + 4 * l], d.out, -1);
    }
    for (int c = 0; c < C; ++c) {
        if (s.ln) {
            add_job(DC_JOB_CROSS_GAMMA, pa.cross[c].G, pa.x0, pa.cst + 4 * c, 4 * C, nullptr, nullptr, G + off[19 + 3 * c], D, c);
            add_job(DC_JOB_SUM, pa.cross[c].G, nullptr, nullptr, 0, nullptr, nullptr, G + off[20 + 3 * c], D, -1);
        }
        add_job(DC_JOB_CROSS_W, pa.cst + 4 * c + 3, pa.x0, c ? pa.cst + 4 * (c - 1) : nullptr, 4 * C, c ? pa.cross[c - 1].gamma : nullptr,
                c ? pa.cross[c - 1].beta : nullptr, G + off[18 + 3 * c], D, c - 1);
    }
    ga.njobs = nj;
    ga.col_blocks = cfirst;
    ga.row_blocks = (int)cdiv64(n, PAIR_WAVES);
    ga.users = users, ga.items = items;
    ga.order_u = pa.order_u, ga.order_i = pa.order_i;
    ga.dx0 = pa.dx0;
    ga.g_users = G + off[0], ga.g_items = G + off[1];
    ga.loss = loss;
    ga.n = (int)n, ga.E = s.E;

    const unsigned grid1 = (unsigned)(pa.tiles + 2 * pa.rank_blocks + pa.zero_blocks);
    if (drop_on) {
        if (s.ln) hipLaunchKernelGGL((dcn_pairs_kernel<true, true, true>), dim3(grid1), dim3(PAIR_THREADS), 0, st, pa, dr);
        else hipLaunchKernelGGL((dcn_pairs_kernel<true, false, true>), dim3(grid1), dim3(PAIR_THREADS), 0, st, pa, dr);
    }
    else if (s.ln) hipLaunchKernelGGL((dcn_pairs_kernel<true, true, false>), dim3(grid1), dim3(PAIR_THREADS), 0, st, pa, dr);
    else hipLaunchKernelGGL((dcn_pairs_kernel<true, false, false>), dim3(grid1), dim3(PAIR_THREADS), 0, st, pa, dr);
    PMGT_LAUNCH_OK();
    const unsigned grid2 = (unsigned)(ga.weight_blocks + ga.col_blocks + 2 * ga.row_blocks);
    if (cross_on) {                                          // (launch 2 draws cross masks only)
        if (s.ln) hipLaunchKernelGGL((dcn_grads_kernel<true, true>), dim3(grid2), dim3(PAIR_THREADS), 0, st, ga, dr);
        else hipLaunchKernelGGL((dcn_grads_kernel<false, true>), dim3(grid2), dim3(PAIR_THREADS), 0, st, ga, dr);
    }
    else if (s.ln) hipLaunchKernelGGL((dcn_grads_kernel<true, false>), dim3(grid2), dim3(PAIR_THREADS), 0, st, ga, dr);
    else hipLaunchKernelGGL((dcn_grads_kernel<false, false>), dim3(grid2), dim3(PAIR_THREADS), 0, st, ga, dr);
    PMGT_LAUNCH_OK();
    return 0;
}

}  // namespace pmgt

using namespace pmgt;

extern "C" {

int64_t pmgt_dcn_layout(int factor_num, int deep_layers, int cross_layers, int use_layer_norm, int64_t user_num, int64_t item_num,
                        int64_t* offsets) {
    DcShape s;
    if (int rc = dc_shape(factor_num, deep_layers, cross_layers, use_layer_norm, user_num, item_num, "pmgt_dcn_layout", &s)) return rc;
    int64_t off[PMGT_DCN_TENSORS];
    const int64_t count = dc_layout(s, off);
    if (offsets)
        for (int i = 0; i < PMGT_DCN_TENSORS; ++i) offsets[i] = off[i];
    return count;
}

int64_t pmgt_dcn_workspace_bytes(int factor_num, int deep_layers, int cross_layers, int use_layer_norm, int64_t n) {
    const char* who = "pmgt_dcn_workspace_bytes";
    DcShape s;
    if (int rc = dc_shape(factor_num, deep_layers, cross_layers, use_layer_norm, 1, 1, who, &s)) return rc;
    if (int rc = pair_check_n(who, n, PMGT_DCN_MAX_PAIRS)) return rc;
    return dc_workspace_floats(s, n) * (int64_t)sizeof(float);
}

int pmgt_dcn_forward(const pmgt_dcn_head* head, const int64_t* users, const int64_t* items, int64_t n, float* logits, void* workspace,
                     int64_t workspace_bytes, void* stream) {
    return dc_run("pmgt_dcn_forward", false, head, users, items, nullptr, n, nullptr, logits, nullptr, workspace, workspace_bytes, stream);
}

int pmgt_dcn_train_grad(const pmgt_dcn_head* head, const int64_t* users, const int64_t* items, const float* labels, int64_t n, float* loss,
                        float* logits, void* workspace, int64_t workspace_bytes, void* stream) {
    return dc_run("pmgt_dcn_train_grad", true, head, users, items, labels, n, loss, logits, nullptr, workspace, workspace_bytes, stream);
}

int pmgt_dcn_train_grad_dropout(const pmgt_dcn_head* head, const int64_t* users, const int64_t* items, const float* labels, int64_t n,
                                float* loss, float* logits, const pmgt_dcn_dropout* drop, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* who = "pmgt_dcn_train_grad_dropout";
    PMGT_CHECK(drop != nullptr, -2, "%s: NULL drop", who);
    return dc_run(who, true, head, users, items, labels, n, loss, logits, drop, workspace, workspace_bytes, stream);
}

}  // extern "C"
