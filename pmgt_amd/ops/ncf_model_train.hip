// Training of the reference's stand-alone NCF class (pmgt/ncf/models.py:14-154, the class ncf.py restates; pmgt_ncf_model_train_grad of
// include/pmgt_capi.h): loss, logits and the gradient of the mean BCE-with-logits loss with respect to every tensor the model's kind trains,
// for n (user, item, label) pairs, in TWO launches.  Kept out of csrc/ for ncf_train.hip's reason.  fp32 end to end; every matrix product
// runs on the exact f32-input MFMA (v_mfma_f32_32x32x2_f32) in the pair-major forms ncf_train.hip states in its header.
//
// WHICH CASES RUN HERE.  A model WITHOUT LayerNorm of kind MLP / NeuMF-end (NeuMF-pre trains as NeuMF-end) is the head ncf_train.hip trains
// over a table: the entry hands it to pmgt_ncf_train_grad / _table / _dropout on the same buffers (the layouts agree), so those bits are
// that file's.  The kernels below cover the LayerNorm layer  h_(l+1) = relu(LN_l(m_l (W_l h_l + b_l)))  and kind GMF
// z = wp . (m_g (gu gi)) + bp, which is the degenerate path with no layer: no MLP tensor is read.
//
// LAUNCH 1, ncf_model_pairs_kernel, three roles by block index (rank and zero as in ncf_train.hip):
//   tile   32 pairs a workgroup of 4 waves.  Per layer: the MFMA product y_l = m_l (W_l x + b_l) (the waves share out the 32-feature
//          blocks; the DROPPED pre-LayerNorm value is stored), a barrier, then ROW WORK: one wave owns a pair's row (at most 256 floats,
//          4 a lane), reduces with a shuffle butterfly and stores (mean, rstd) and h_(l+1) = relu(xhat gamma + beta).  Then the GMF
//          product, the predict layer, the stable loss and dlogit.  Back: row work g = dh (h > 0) (stored: gamma / beta read g and xhat),
//          dy = m_l LNbwd(g) = m_l rstd ((g gamma - mean(g gamma)) - xhat mean(g gamma xhat)), a barrier, the MFMA data product
//          dh_(l-1) = dy W_l, down to dx [n][2 d] = m_e (dy_0 W_0).  The layer mask is drawn again on the way back; nothing of it is stored.
//          FOUR CHAINS: the k-steps of every layer product are dealt in turn onto four MFMA accumulators, and the predict layer's dot
//          onto four sums a lane, joined as (a + b) + (c + d).  One chain of K / 2 dependent steps (256 at K = 512) left the widest model
//          3 to 5.7 x above the error of the same formula in fp32 numpy, whose sums are blocked; four chains of K / 8 come to 2.1 x at most.
//   rank   the position of every pair in the STABLE order by user id and by item id, counted
//   zero   the gradient rows of the embedding tables, whole, and as a second range the gradient of embed_item_MLP when it is trained
// LAUNCH 2, ncf_model_grads_kernel, three roles:
//   weight one workgroup per 32 x 32 block of a layer's dW = dy^T h, the constant column for the bias gradient, the predict layer the
//          pseudo-layer with dz = [dlogit, loss_pair]: ncf_train.hip's role
//   cols   64 columns of one layer a workgroup: d gamma = sum_p g xhat and d beta = sum_p g, xhat recomputed from the stored y and
//          (mean, rstd) by launch 1's sequence of operations (the file is compiled without contraction, so the bits agree); wave a sums
//          the pairs a, a + 4, .. in order and the four partial sums are added as (w0 + w1) + (w2 + w3)
//   rows   one wave per position of the stable order: the segment sums of the per-pair embedding rows in pair order
// DETERMINISM: no atomic anywhere; every sum has one fixed order, so the same inputs give the same bits, on other buffers and another
// workspace too.  Rows no pair touches keep the +0.0 of launch 1.
// DROPOUT: ncf_train.hip's sites and RNG: emb on the 16-byte x loads of layer 0 (drawn again by the weight task of layer 0 and by the last
// data gradient), layer l on y_l before its store (drawn again for dy_l), gmf on the GMF product.  A site whose p is 0 draws nothing; with
// every p 0 no dropout instantiation is launched.
#include <climits>
#include <cmath>

#include "ncf_head.h"

#pragma clang fp contract(off)

namespace pmgt {

static constexpr int NM_THREADS = 256, NM_WAVES = 4, NM_TILE = 32, NM_MAX_LAYERS = PMGT_NCF_MAX_LAYERS;
static constexpr int NM_ZERO_BLOCKS = 1024, NM_MAX_TASKS = NM_MAX_LAYERS + 1;

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

struct NmSrc {      // a matrix [n][w1 + w2] given by one or two row sources, each read by the pair index (idx NULL) or through an id list
    const float* p1;
    const int64_t* idx1;
    int w1;
    const float* p2;
    const int64_t* idx2;
    int w2;
};

struct NmTask {
    const float* a;      // dz [n][m]
    NmSrc b;             // the layer's input [n][k]
    float* gw;           // [m][k]
    float* gb;           // [m]
    int m, col_blocks, first, predict;      // col_blocks counts the constant column's block
};

struct NmJob {           // cols: d gamma and d beta of one layer
    const float *g, *y, *stat;
    float *ggamma, *gbeta;
    int W, first;
};

typedef pmgt_ncf_dropout NmDrop;

struct NmGradsArgs {
    NmTask task[NM_MAX_TASKS];
    NmJob job[NM_MAX_LAYERS];
    const int64_t *users, *items;
    const int *order_u, *order_i;
    const float *dx, *ggu, *ggi;
    float *g_u_mlp, *g_gu, *g_gi, *g_table, *loss;      // g_table: the gradient of a trained embed_item_MLP, else NULL
    int n, d, factor, gmf, mlp, ntasks, njobs, weight_blocks, col_blocks, row_blocks;
};

__device__ __forceinline__ float4 nm_ld4(const float* p, bool ok) {
    return ok ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ float nm_elem(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
__device__ __forceinline__ int nm_wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
__device__ __forceinline__ DropKey nm_drop_off() { return DropKey{0u, 0u, 0u, 1.f, false}; }
__device__ __forceinline__ void nm_mul4(float4& v, const float (&m)[4]) { v.x *= m[0], v.y *= m[1], v.z *= m[2], v.w *= m[3]; }
__device__ __forceinline__ float nm_wave_sum(float x) {      // a butterfly: every lane ends with the same bits
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// a = (a + b) + (c + d): the four accumulators of a product whose k-steps were dealt out in turn.  A chain of K / 8 MFMA steps instead of K / 2
// keeps the rounding error of the widest layers (K = 512) near that of a blocked host sum, and four independent chains keep the MFMA pipe busy
__device__ __forceinline__ void nm_join(f32x16& a, const f32x16& b, const f32x16& c, const f32x16& d) {
#pragma unroll
    for (int g = 0; g < 16; ++g) a[g] = (a[g] + b[g]) + (c[g] + d[g]);
}

// y[pair][0 .. M) = W [M][K] x + bias, NO activation; x = [r1[0 .. w1) ; r2[0 .. K - w1)], the lane's own pair row(s)
// DROP: x is multiplied by the mask of key kx as it is loaded and the result by the mask of ky before the store (row = the pair)
template <bool DROP>
__device__ __forceinline__ void nm_forward(const float* __restrict__ W, const float* __restrict__ bias, int M, int K, const float* r1, int w1,
                                           const float* r2, bool valid, float* y_row, int wave, int lane, const DropKey& kx, const DropKey& ky,
                                           int pair) {
    const int p = lane & 31, h = lane >> 5;
    for (int mb = wave; mb * 32 < M; mb += NM_WAVES) {
        f32x16 acc, acc1, acc2, acc3;                        // k-step t adds into accumulator t & 3: four chains of K / 8 steps (nm_join)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int f = mb * 32 + rho(g) + 4 * h;
            acc[g] = f < M ? bias[f] : 0.f;
            acc1[g] = acc2[g] = acc3[g] = 0.f;
        }
        const int m = mb * 32 + p;
        const float* wrow = W + (int64_t)m * K;
        for (int k0 = 0; k0 < K; k0 += 32) {
            float4 a[4], x[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + 16 * h + 4 * j;
                a[j] = nm_ld4(wrow + k, m < M && k < K);
                x[j] = nm_ld4(k < w1 ? r1 + k : r2 + (k - w1), valid && k < K);
                if constexpr (DROP) {
                    if (kx.on) {
                        float mk[4];
                        drop_mul4(kx, (uint32_t)pair, (uint32_t)(k >> 2), mk);
                        nm_mul4(x[j], mk);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].x, x[j].x, acc, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].y, x[j].y, acc1, 0, 0, 0);
                acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].z, x[j].z, acc2, 0, 0, 0);
                acc3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j].w, x[j].w, acc3, 0, 0, 0);
            }
        }
        nm_join(acc, acc1, acc2, acc3);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int f = mb * 32 + 8 * q + 4 * h;
            float4 v = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
            if constexpr (DROP) {
                if (ky.on) {
                    float mk[4];
                    drop_mul4(ky, (uint32_t)pair, (uint32_t)(f >> 2), mk);
                    nm_mul4(v, mk);
                }
            }
            if (valid && f < M) *reinterpret_cast<float4*>(y_row + f) = v;
        }
    }
}

// dx[pair][c] = sum_o W[o][c] dz[pair][o] for c in [0, C), W [M][K] with C <= K.  DROP: the result is multiplied by the mask of kx
template <bool DROP>
__device__ __forceinline__ void nm_backward(const float* __restrict__ W, int M, int K, int C, const float* dz_row, bool valid, float* dx_row,
                                            int wave, int lane, const DropKey& kx, int pair) {
    const int p = lane & 31, h = lane >> 5;
    for (int cb = wave; cb * 32 < C; cb += NM_WAVES) {
        f32x16 acc, acc1, acc2, acc3;                        // (four chains, as in nm_forward)
#pragma unroll
        for (int g = 0; g < 16; ++g) acc[g] = acc1[g] = acc2[g] = acc3[g] = 0.f;
        const int c = cb * 32 + p;
        for (int o0 = 0; o0 < M; o0 += 32) {
            float4 z[4];
            float a[16];
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = nm_ld4(dz_row + o0 + 16 * h + 4 * j, valid && o0 + 16 * h + 4 * j < M);
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int o = o0 + 16 * h + s;
                a[s] = (c < C && o < M) ? W[(int64_t)o * K + c] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * j], z[j].x, acc, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * j + 1], z[j].y, acc1, 0, 0, 0);
                acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * j + 2], z[j].z, acc2, 0, 0, 0);
                acc3 = __builtin_amdgcn_mfma_f32_32x32x2f32(a[4 * j + 3], z[j].w, acc3, 0, 0, 0);
            }
        }
        nm_join(acc, acc1, acc2, acc3);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int f = cb * 32 + 8 * q + 4 * h;
            float4 v = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
            if constexpr (DROP) {
                if (kx.on) {
                    float mk[4];
                    drop_mul4(kx, (uint32_t)pair, (uint32_t)(f >> 2), mk);
                    nm_mul4(v, mk);
                }
            }
            if (valid && f < C) *reinterpret_cast<float4*>(dx_row + f) = v;
        }
    }
}

template <bool DROP>
__global__ __launch_bounds__(NM_THREADS) void ncf_model_pairs_kernel(NmPairsArgs a, NmDrop dr) {
    __shared__ float s_dl[NM_TILE];
    __shared__ int64_t s_ids[NM_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = nm_wave_index(), n = a.n;
    int bid = blockIdx.x;
    if (bid >= a.tiles + 2 * a.rank_blocks) {                // ---- zero: the embedding gradients, whole
        float4* z = reinterpret_cast<float4*>(a.zero_base);
        float4* z2 = reinterpret_cast<float4*>(a.zero2_base);
        const int64_t total = a.zero_vec4 + a.zero2_vec4;
        for (int64_t i = (int64_t)(bid - a.tiles - 2 * a.rank_blocks) * NM_THREADS + tid; i < total; i += (int64_t)a.zero_blocks * NM_THREADS) {
            if (i < a.zero_vec4) z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            else z2[i - a.zero_vec4] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    if (bid >= a.tiles) {                                    // ---- rank: the stable order by id, counted
        bid -= a.tiles;
        const int kind = bid / a.rank_blocks;
        const int64_t* ids = kind ? a.items : a.users;
        int* order = kind ? a.order_i : a.order_u;
        const int p = (bid - kind * a.rank_blocks) * NM_THREADS + tid;
        const int64_t mine = p < n ? ids[p] : 0;
        int rank = 0;
        for (int q0 = 0; q0 < n; q0 += NM_THREADS) {
            __syncthreads();
            s_ids[tid] = q0 + tid < n ? ids[q0 + tid] : 0;
            __syncthreads();
            const int cnt = min(NM_THREADS, n - q0);
            for (int j = 0; j < cnt; ++j) {
                const int64_t v = s_ids[j];
                rank += (v < mine || (v == mine && q0 + j < p)) ? 1 : 0;
            }
        }
        if (p < n) order[rank] = p;
        return;
    }
    // ---- tile: forward and data gradient of 32 pairs
    const int d = a.d, F = a.factor, L = a.num_layers;
    const int pl = lane & 31, h = lane >> 5;
    const int pair = bid * NM_TILE + pl;
    const bool valid = pair < n;
    const int64_t uid = valid ? a.users[pair] : 0, iid = valid ? a.items[pair] : 0;
    DropKey kemb = nm_drop_off(), kgmf = nm_drop_off();
    if constexpr (DROP) {
        if (L) kemb = make_drop_key(DropCfg{dr.rng, dr.p_emb, NCF_SITE_EMB});
        if (a.gmf) kgmf = make_drop_key(DropCfg{dr.rng, dr.p_emb, NCF_SITE_GMF});
    }
    for (int l = 0; l < L; ++l) {
        const NmLayer& ly = a.layer[l];
        const int M = ly.out;
        DropKey klay = nm_drop_off();
        if constexpr (DROP) klay = make_drop_key(DropCfg{dr.rng, dr.p_layer[l], NCF_SITE_LAYER + (uint32_t)l});
        if (l == 0)
            nm_forward<DROP>(ly.w, ly.b, d, 2 * d, a.u_mlp + uid * d, d, a.table + iid * d, valid, ly.y + (int64_t)pair * d, wave, lane, kemb, klay,
                             pair);
        else
            nm_forward<DROP>(ly.w, ly.b, M, 2 * M, a.layer[l - 1].h + (int64_t)pair * 2 * M, 2 * M, nullptr, valid, ly.y + (int64_t)pair * M, wave,
                             lane, nm_drop_off(), klay, pair);
        __syncthreads();
        const float inv = 1.f / (float)M;
        for (int pp = wave; pp < NM_TILE; pp += NM_WAVES) {  // row work: LayerNorm and ReLU, a wave a row
            const int pr = bid * NM_TILE + pp;
            if (pr >= n) break;                              // (uniform per wave)
            const float* yrow = ly.y + (int64_t)pr * M;
            float v[4], c[4], s = 0.f, q = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int f = lane + 64 * j;
                v[j] = f < M ? yrow[f] : 0.f;
                s += v[j];
            }
            const float mean = nm_wave_sum(s) * inv;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                c[j] = lane + 64 * j < M ? v[j] - mean : 0.f;
                q += c[j] * c[j];
            }
            const float rstd = 1.f / sqrtf(nm_wave_sum(q) * inv + a.eps);
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
                const float z = s + a.bp[0], y = a.labels[pair];
                const float e = expf(-fabsf(z));
                const float sig = z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
                dl = (sig - y) / (float)n;
                if (a.logits) a.logits[pair] = z;
                a.pz[(int64_t)pair * 2] = dl;
                a.pz[(int64_t)pair * 2 + 1] = fmaxf(z, 0.f) - z * y + log1pf(e);
            }
            s_dl[pl] = dl;
        }
    }
    __syncthreads();
    if (a.gmf) {
        for (int e = tid; e < NM_TILE * F; e += NM_THREADS) {    // the per-pair GMF gradients
            const int pp = e / F, f = e - pp * F, pr = bid * NM_TILE + pp;
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
        DropKey klay = nm_drop_off();
        if constexpr (DROP) klay = make_drop_key(DropCfg{dr.rng, dr.p_layer[l], NCF_SITE_LAYER + (uint32_t)l});
        const float inv = 1.f / (float)M;
        for (int pp = wave; pp < NM_TILE; pp += NM_WAVES) {  // row work: g = dh (h > 0), dy = m LNbwd(g)
            const int pr = bid * NM_TILE + pp;
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
            const float m1 = nm_wave_sum(s1) * inv, m2 = nm_wave_sum(s2) * inv;
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
            nm_backward<DROP>(ly.w, M, 2 * M, 2 * M, ly.dz + (int64_t)pair * M, valid, a.layer[l - 1].g + (int64_t)pair * 2 * M, wave, lane,
                              nm_drop_off(), pair);
        else
            nm_backward<DROP>(ly.w, d, 2 * d, 2 * d, ly.dz + (int64_t)pair * d, valid, a.dx + (int64_t)pair * 2 * d, wave, lane, kemb, pair);
        __syncthreads();
    }
}

__device__ __forceinline__ float nm_src_at(const NmSrc& s, int pair, int c) {
    if (c < s.w1) {
        const int64_t row = s.idx1 ? s.idx1[pair] : pair;
        return s.p1[row * s.w1 + c];
    }
    const int64_t row = s.idx2 ? s.idx2[pair] : pair;
    return s.p2[row * s.w2 + (c - s.w1)];
}

// DROP: the weight task of layer 0 gathers its B operand from the tables and applies the emb mask to it, drawn again per element
template <bool DROP>
__global__ __launch_bounds__(NM_THREADS) void ncf_model_grads_kernel(NmGradsArgs a, NmDrop dr) {
    __shared__ float s_acc[NM_WAVES][16][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = nm_wave_index(), n = a.n;
    int bid = blockIdx.x;
    if (bid >= a.weight_blocks + a.col_blocks) {             // ---- rows: segment sums of the per-pair embedding gradients in pair order
        bid -= a.weight_blocks + a.col_blocks;
        const int kind = bid / a.row_blocks;
        const int s = (bid - kind * a.row_blocks) * NM_WAVES + wave;
        if (s >= n) return;
        const int64_t* ids = kind ? a.items : a.users;
        const int* order = kind ? a.order_i : a.order_u;
        const int64_t id = ids[order[s]];
        if (s > 0 && ids[order[s - 1]] == id) return;        // (uniform per wave) not the start of a run
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
            float sum = 0.f;
            for (int t = s; t < n; ++t) {
                const int pr = order[t];
                if (ids[pr] != id) break;
                sum += src[(int64_t)pr * sw + cc];
            }
            dst[id * w + cc] = sum;
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
        for (int p = wave; p < n; p += NM_WAVES) {
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
    int ti = 0;
    for (int i = 1; i < a.ntasks; ++i)
        if (bid >= a.task[i].first) ti = i;
    const NmTask& t = a.task[ti];
    const int local = bid - t.first, M = t.m, K = t.b.w1 + t.b.w2;
    const int mb = local / t.col_blocks, nb = local - mb * t.col_blocks;
    const bool ones = nb == t.col_blocks - 1;
    const int p = lane & 31, h = lane >> 5, m = mb * 32 + p, c = nb * 32 + p;
    DropKey kemb = nm_drop_off();
    if constexpr (DROP) {
        if (ti == 0 && !t.predict && !ones) kemb = make_drop_key(DropCfg{dr.rng, dr.p_emb, NCF_SITE_EMB});
    }
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.f;
    for (int ch = wave; ch * 32 < n; ch += NM_WAVES) {
        float av[16], bv[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int pair = ch * 32 + 16 * h + s;
            const bool ok = pair < n;
            av[s] = (ok && m < M) ? t.a[(int64_t)pair * M + m] : 0.f;
            bv[s] = ones ? (p == 0 ? 1.f : 0.f) : ((ok && c < K) ? nm_src_at(t.b, pair, c) : 0.f);
            if constexpr (DROP) {
                if (kemb.on) bv[s] *= drop_mul1(kemb, (uint32_t)pair, (uint32_t)c);
            }
        }
#pragma unroll
        for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc, 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < 16; ++g) s_acc[wave][g][lane] = acc[g];
    __syncthreads();
    const int gq = tid >> 6;
#pragma unroll
    for (int gg = 0; gg < 4; ++gg) {
        const int g = gq * 4 + gg;
        const float v = (s_acc[0][g][lane] + s_acc[1][g][lane]) + (s_acc[2][g][lane] + s_acc[3][g][lane]);
        const int mo = mb * 32 + rho(g) + 4 * h;
        if (t.predict) {
            if (mo == 0) {
                if (ones) { if (p == 0) t.gb[0] = v; }
                else if (c < K) t.gw[c] = v;
            } else if (mo == 1 && ones && p == 0) {
                a.loss[0] = v / (float)n;
            }
        } else if (mo < M) {
            if (ones) { if (p == 0) t.gb[mo] = v; }
            else if (c < K) t.gw[(int64_t)mo * K + c] = v;
        }
    }
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
    PMGT_CHECK(user_num >= 1 && user_num <= 0x7FFFFFFELL, -2, "%s: user_num = %lld outside [1, 2^31 - 2]", who, (long long)user_num);
    PMGT_CHECK(item_num >= 1 && item_num <= 0x7FFFFFFELL, -2, "%s: item_num = %lld outside [1, 2^31 - 2]", who, (long long)item_num);
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
    PMGT_CHECK(n >= 1 && n <= PMGT_NCF_TRAIN_MAX_PAIRS, -2, "%s: n = %lld pairs outside [1, %d]", who, (long long)n, PMGT_NCF_TRAIN_MAX_PAIRS);
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
    PMGT_CHECK(n >= 1 && n <= PMGT_NCF_TRAIN_MAX_PAIRS, -2, "%s: n = %lld pairs outside [1, %d]", who, (long long)n, PMGT_NCF_TRAIN_MAX_PAIRS);
    PMGT_CHECK((!s.mlp || m->item_table) && m->params && m->grads && users && items && labels && loss && workspace, -2, "%s: NULL buffer", who);
    PMGT_CHECK(!s.table || m->table_grad, -2, "%s: NULL table_grad", who);
    const uintptr_t table_bits = s.mlp ? (uintptr_t)m->item_table | (s.table ? (uintptr_t)m->table_grad : 0) : 0;
    PMGT_CHECK(((table_bits | (uintptr_t)m->params | (uintptr_t)m->grads | (uintptr_t)workspace) & 15) == 0, -2,
               "%s: the item table, the parameters, the gradients (the table's included) and the workspace must be 16-byte aligned", who);
    PMGT_CHECK((((uintptr_t)labels | (uintptr_t)loss | (uintptr_t)logits) & 3) == 0 && (((uintptr_t)users | (uintptr_t)items) & 7) == 0, -2,
               "%s: misaligned buffer", who);
    const int64_t need = pmgt_ncf_model_workspace_bytes(m->factor_num, m->num_layers, m->kind, m->use_layer_norm, m->train_items, n);
    PMGT_CHECK(workspace_bytes >= need, -2, "%s: workspace of %lld bytes below the %lld needed", who, (long long)workspace_bytes, (long long)need);
    NmDrop dr = {};
    bool drop_on = false;                                    // every p 0: the instantiations without dropout
    if (drop) {
        dr.rng = drop->rng, dr.p_emb = drop->p_emb;
        PMGT_CHECK(dr.p_emb >= 0.f && dr.p_emb < 1.f, -2, "%s: p_emb = %g outside [0, 1)", who, (double)dr.p_emb);      // (a NaN fails both)
        drop_on = dr.p_emb > 0.f;
        for (int l = 0; l < s.L; ++l) {
            dr.p_layer[l] = drop->p_layer[l];
            PMGT_CHECK(dr.p_layer[l] >= 0.f && dr.p_layer[l] < 1.f, -2, "%s: p_layer[%d] = %g outside [0, 1)", who, l, (double)dr.p_layer[l]);
            drop_on = drop_on || dr.p_layer[l] > 0.f;
        }
        PMGT_CHECK(!drop_on || (dr.rng && ((uintptr_t)dr.rng & 7) == 0), -2, "%s: dropout needs the device {seed, step} pair, 8-byte aligned", who);
    }
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
    pa.tiles = (int)cdiv64(n, NM_TILE);
    pa.rank_blocks = (int)cdiv64(n, NM_THREADS);
    pa.zero_blocks = (int)std::min<int64_t>(NM_ZERO_BLOCKS, cdiv64(pa.zero_vec4 + pa.zero2_vec4, NM_THREADS));

    int first = 0;
    for (int l = 0; l < L; ++l) {
        const int out = d >> l;
        NmTask& t = ga.task[l];
        t.a = pa.layer[l].dz;
        t.m = out;
        if (l == 0) t.b = NmSrc{pa.u_mlp, users, d, pa.table, items, d};
        else t.b = NmSrc{pa.layer[l - 1].h, nullptr, 2 * out, nullptr, nullptr, 0};
        t.gw = G + off[3 + 4 * l];
        t.gb = G + off[4 + 4 * l];
        t.col_blocks = (2 * out + 31) / 32 + 1;
        t.first = first;
        t.predict = 0;
        first += (out + 31) / 32 * t.col_blocks;
    }
    {
        NmTask& t = ga.task[L];
        t.a = pa.pz;
        t.m = 2;
        if (s.gmf && L) t.b = NmSrc{pa.gprod, nullptr, F, pa.layer[L - 1].h, nullptr, F};
        else if (L) t.b = NmSrc{pa.layer[L - 1].h, nullptr, F, nullptr, nullptr, 0};
        else t.b = NmSrc{pa.gprod, nullptr, F, nullptr, nullptr, 0};
        t.gw = G + off[NM_OFF_WP];
        t.gb = G + off[NM_OFF_BP];
        t.col_blocks = (((s.gmf && L) ? 2 * F : F) + 31) / 32 + 1;
        t.first = first;
        t.predict = 1;
        first += t.col_blocks;
    }
    ga.ntasks = L + 1;
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
    ga.row_blocks = (int)cdiv64(n, NM_WAVES);
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
    if (drop_on) hipLaunchKernelGGL((ncf_model_pairs_kernel<true>), dim3(grid1), dim3(NM_THREADS), 0, st, pa, dr);
    else hipLaunchKernelGGL((ncf_model_pairs_kernel<false>), dim3(grid1), dim3(NM_THREADS), 0, st, pa, dr);
    PMGT_LAUNCH_OK();
    const unsigned grid2 = (unsigned)(ga.weight_blocks + ga.col_blocks + kinds * ga.row_blocks);
    if (drop_on && L && dr.p_emb > 0.f) hipLaunchKernelGGL((ncf_model_grads_kernel<true>), dim3(grid2), dim3(NM_THREADS), 0, st, ga, dr);
    else hipLaunchKernelGGL((ncf_model_grads_kernel<false>), dim3(grid2), dim3(NM_THREADS), 0, st, ga, dr);
    PMGT_LAUNCH_OK();
    return 0;
}

}  // extern "C"
