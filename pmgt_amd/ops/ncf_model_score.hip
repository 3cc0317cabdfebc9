// Fused scoring of a batch of users against the whole catalogue by the eval-mode head of the reference's stand-alone NCF class
// (pmgt_ncf_model_score of include/pmgt_capi.h; the class: pmgt/ncf/models.py:14-154, restated in pmgt_amd/ncf.py).  Kept out of csrc/ for
// eval_metrics.hip's reason.  fp32 end to end, no atomic, one float stored per pair, the same bits for the same inputs.
//
// WHICH CASES RUN HERE.  A model WITHOUT LayerNorm of kind MLP / NeuMF-end / NeuMF-pre is the head ncf_score.hip scores: the entry hands it
// to pmgt_ncf_score, so those bits are that file's.  The kernels below cover the LayerNorm layer  h_(l+1) = relu(LN_l(W_l h_l + b_l))  and
// kind GMF.  The MLP tower keeps ncf_score.hip's design (its header: layer 0 split into Pu [n][d] and Pi [I][d] by the caller, every layer
// transposed on the exact f32-input 32x32x2 MFMA, the activations of a pair chained in the registers of its lane, the weights streamed
// through LDS in chunks of 32 k-columns, 32 items x 4 UW users a workgroup) and shares ncf_score_tile.h with it: the chunk transfers, the
// bias and the predict layer.  What is new:
//   LAYER 0.   The pre-norm row of a pair is y = Pu[r] + Pi[j], formed on the fly from the LDS tiles.  Before the k-loop every lane computes
//              its pair's mean and rstd over the d features: lane half h sums the features [h d / 2, (h + 1) d / 2) in order, the halves
//              exchange once (a + b and b + a are the same float, so both halves hold the same bits), then the same for the squared
//              deviations.  The k-loop feeds relu(((y - mean) rstd) gamma0[k] + beta0[k]); gamma0 / beta0 sit in LDS.
//   LAYER l.   The M = d >> l outputs of a pair sit in the 16 registers x NB blocks of its lane and of the lane of the other half: the
//              statistics are a register sum plus one exchange, before the ReLU.  The blocks are zero-padded to 32 features; features past
//              M take no part in either sum, the divisor is M, and they are written back as 0.
//   NUMERICS.  ncf_model_train.hip's: two passes (the mean, then the sum of squared deviations), biased variance, rstd = 1 / sqrt(var +
//              eps), the file compiled without contraction.  The products keep ONE accumulation chain: K is at most 256 here (that
//              file's K = 512 needed four): the k-ordered chain emulated on the host stays within 1.5 x the fp32 formula's error at d = 256,
//              dealing the steps onto two or four accumulators gains nothing there, and the device gives 1.62 x at most (the bound is 4 x).
//   NaN.       A pair's values live on the two lanes of its item only (the MFMA's B column, the one exchange with lane ^ 32), and the ReLU
//              keeps a NaN: a NaN in a row of Pi reaches every score of that item and no other.
//   L = 1.     One pair a thread (ncf_score.hip's VALU kernel) with the LayerNorm over the F features in front of the predict dot.
//   GMF.       scores[r][j] = sum_f wp[f] (gu[users[r]][f] gi[j][f]) + bp: one item a thread, its gi row in registers, 8 users a workgroup
//              (their gu rows are uniform loads), the dot dealt onto four sums joined as (a + b) + (c + d).  No MLP tensor is read.
#include <cmath>

#pragma clang fp contract(off)

#include "ncf_score_tile.h"

namespace pmgt {

static constexpr int NMS_GMF_USERS = 8;                                     // users a workgroup of the GMF kernel

struct NmsArgs {
    const float* w[NCF_MAX_LAYERS];      // [i]: W_i [d >> i][d >> (i - 1)]; [0] is never read (the caller's split)
    const float* b[NCF_MAX_LAYERS];
    const float* gamma[NCF_MAX_LAYERS];  // LayerNorm of layer i over d >> i features
    const float* beta[NCF_MAX_LAYERS];
    const float* wp;                     // predict_layer.weight [factor] or, with both branches, [2 factor] = [gmf | mlp]
    const float* bp;
    const float* gu;                     // embed_user_GMF.weight [user_num][factor] or NULL
    const float* gi;                     // embed_item_GMF.weight [I][factor] or NULL
    const float* pu;                     // [n][d]
    const float* pi;                     // [I][d]
    const int64_t* users;                // [n]
    float* scores;                       // [n][row_stride]
    int64_t row_stride, user_num;
    float eps;
    int n, n_items, d, factor, num_layers, item_tiles;
};

// acc = relu(LN(acc)) over the M true features of every pair (feature 32 mb + rho(g) + 4 h of pair p in acc[u][mb][g], the other half of the
// features on lane ^ 32); features past M come out as 0
template <int UW, int NB>
__device__ __forceinline__ void nms_ln_relu(f32x16 (&acc)[UW][NB], const float* __restrict__ gamma, const float* __restrict__ beta, int M, float eps,
                                            int h) {
    const float inv = 1.f / (float)M;                        // (M is a power of two: the product is the quotient)
    float mean[UW], rstd[UW];
#pragma unroll
    for (int u = 0; u < UW; ++u) {
        float s = 0.f;
#pragma unroll
        for (int mb = 0; mb < NB; ++mb)
#pragma unroll
            for (int g = 0; g < 16; ++g)
                if (mb * 32 + rho(g) + 4 * h < M) s += acc[u][mb][g];
        s += __shfl_xor(s, 32, 64);
        mean[u] = s * inv;
        float q = 0.f;
#pragma unroll
        for (int mb = 0; mb < NB; ++mb)
#pragma unroll
            for (int g = 0; g < 16; ++g)
                if (mb * 32 + rho(g) + 4 * h < M) {
                    const float c = acc[u][mb][g] - mean[u];
                    q += c * c;
                }
        q += __shfl_xor(q, 32, 64);
        rstd[u] = 1.f / sqrtf(q * inv + eps);
    }
#pragma unroll
    for (int mb = 0; mb < NB; ++mb)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int f = mb * 32 + rho(g) + 4 * h;
            const bool live = f < M;
            const float ga = live ? gamma[f] : 0.f, be = live ? beta[f] : 0.f;
#pragma unroll
            for (int u = 0; u < UW; ++u) acc[u][mb][g] = live ? relu_keep_nan(((acc[u][mb][g] - mean[u]) * rstd[u]) * ga + be) : 0.f;
        }
}

// Y = relu(LN(W X + bias)) for a layer whose input X sits in the accumulators of the previous one: K true inputs (X is zero past them), M outputs
template <int UW, int NBI, int NBO>
__device__ __forceinline__ void nms_layer_from_acc(const f32x16 (&X)[UW][NBI], f32x16 (&Y)[UW][NBO], const NmsArgs& a, int layer, float* ws, int tid) {
    const int lane = tid & 63, p = lane & 31, h = lane >> 5;
    const int M = a.d >> layer, K = a.d >> (layer - 1);
    const float* __restrict__ W = a.w[layer];
    bias_init<UW, NBO>(Y, a.b[layer], M, h);
    float st[NBO * 4];
    chunk_fetch<NBO>(st, W, M, K, 0, tid);
#pragma unroll
    for (int b = 0; b < NBI; ++b) {
        if (b * 32 >= K) break;                      // (uniform)
        __syncthreads();                             // every wave is done with the previous chunk
        chunk_store<NBO>(st, ws, tid);
        __syncthreads();
        if ((b + 1) * 32 < K && b + 1 < NBI) chunk_fetch<NBO>(st, W, M, K, (b + 1) * 32, tid);
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            if (b * 32 + rho(g) >= K) continue;      // (uniform) k-steps wholly past the true width
            float wa[NBO];
#pragma unroll
            for (int mb = 0; mb < NBO; ++mb) wa[mb] = ws[(mb * 32 + p) * NCF_CHUNK_STRIDE + rho(g) + 4 * h];
#pragma unroll
            for (int u = 0; u < UW; ++u)
#pragma unroll
                for (int mb = 0; mb < NBO; ++mb) Y[u][mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[mb], X[u][b][g], Y[u][mb], 0, 0, 0);
        }
    }
    nms_ln_relu<UW, NBO>(Y, a.gamma[layer], a.beta[layer], M, a.eps, h);
}

// the layers behind `layer - 1`, halving the block count while it is above one, then the predict layer
template <int UW, int NBI>
__device__ __forceinline__ void nms_run_tail(f32x16 (&X)[UW][NBI], int layer, const NmsArgs& a, const NcfTile& t, float* ws, int tid) {
    if constexpr (NBI > 1) {
        if (layer < a.num_layers) {
            f32x16 Y[UW][NBI / 2];
            nms_layer_from_acc<UW, NBI, NBI / 2>(X, Y, a, layer, ws, tid);
            nms_run_tail<UW, NBI / 2>(Y, layer + 1, a, t, ws, tid);
        } else {
            predict_store<UW, NBI>(X, a, t);
        }
    } else {
        for (; layer < a.num_layers; ++layer) {
            f32x16 Y[UW][1];
            nms_layer_from_acc<UW, 1, 1>(X, Y, a, layer, ws, tid);
#pragma unroll
            for (int u = 0; u < UW; ++u) X[u][0] = Y[u][0];
        }
        predict_store<UW, 1>(X, a, t);
    }
}

// NB = 32-row blocks of layer 1's output (d / 2 rounded up to 32); dynamic LDS: Pi tile | Pu tile | GMF item tile | gamma0 | beta0 | weight chunk
template <int UW, int NB> __global__ __launch_bounds__(NCF_THREADS) void ncf_model_score_kernel(NmsArgs a) {
    extern __shared__ __align__(16) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = lane & 31, h = lane >> 5;
    const int d = a.d, F = a.factor, TU = NCF_WAVES * UW;
    float* pi_s = smem;                                      // [32][d + 1]
    float* pu_s = pi_s + NCF_ITEMS * (d + 1);                // [TU][d]
    float* gi_s = pu_s + TU * d;                             // [32][F + 1]
    float* g0_s = gi_s + NCF_ITEMS * (F + 1);                // [d]
    float* b0_s = g0_s + d;                                  // [d]
    float* ws = b0_s + d;                                    // [32 NB][33]
    NcfTile t;
    t.j0 = (int)(blockIdx.x % (unsigned)a.item_tiles) * NCF_ITEMS;
    t.r0 = (int)(blockIdx.x / (unsigned)a.item_tiles) * TU;
    t.wave = wave;
    t.lane = lane;
    t.gi_s = gi_s;
    // rows outside the batch / the catalogue are zeros: computed, never stored
    for (int e = tid; e < NCF_ITEMS * d; e += NCF_THREADS) {
        const int row = e / d, c = e - row * d, j = t.j0 + row;
        pi_s[row * (d + 1) + c] = j < a.n_items ? a.pi[(int64_t)j * d + c] : 0.f;
    }
    for (int e = tid; e < TU * d; e += NCF_THREADS) {
        const int row = e / d, c = e - row * d, r = t.r0 + row;
        pu_s[e] = r < a.n ? a.pu[(int64_t)r * d + c] : 0.f;
    }
    if (a.gi)
        for (int e = tid; e < NCF_ITEMS * F; e += NCF_THREADS) {
            const int row = e / F, c = e - row * F, j = t.j0 + row;
            gi_s[row * (F + 1) + c] = j < a.n_items ? a.gi[(int64_t)j * F + c] : 0.f;
        }
    for (int e = tid; e < d; e += NCF_THREADS) g0_s[e] = a.gamma[0][e], b0_s[e] = a.beta[0][e];
    __syncthreads();                                         // the tiles are written
    // the statistics of layer 0's row y = Pu[r] + Pi[j] of every pair of the lane: each half sums its half of the features, one exchange
    const float* pu_w = pu_s + wave * UW * d;
    const float* pi_row = pi_s + p * (d + 1);
    const int half = d >> 1, f0 = h * half;
    const float inv = 1.f / (float)d;                        // (d is a power of two)
    float mean[UW], rstd[UW];
    {
        float s[UW];
#pragma unroll
        for (int u = 0; u < UW; ++u) s[u] = 0.f;
        for (int k = f0; k < f0 + half; k += 4) {            // (half is a multiple of 8; the Pu rows are 16-byte aligned in LDS)
            const float pv[4] = {pi_row[k], pi_row[k + 1], pi_row[k + 2], pi_row[k + 3]};
#pragma unroll
            for (int u = 0; u < UW; ++u) {
                const float4 uv = *reinterpret_cast<const float4*>(pu_w + u * d + k);
                s[u] += uv.x + pv[0], s[u] += uv.y + pv[1], s[u] += uv.z + pv[2], s[u] += uv.w + pv[3];
            }
        }
#pragma unroll
        for (int u = 0; u < UW; ++u) {
            s[u] += __shfl_xor(s[u], 32, 64);
            mean[u] = s[u] * inv;
            s[u] = 0.f;
        }
        for (int k = f0; k < f0 + half; k += 4) {
            const float pv[4] = {pi_row[k], pi_row[k + 1], pi_row[k + 2], pi_row[k + 3]};
#pragma unroll
            for (int u = 0; u < UW; ++u) {
                const float4 uv = *reinterpret_cast<const float4*>(pu_w + u * d + k);
                const float c0 = (uv.x + pv[0]) - mean[u], c1 = (uv.y + pv[1]) - mean[u], c2 = (uv.z + pv[2]) - mean[u], c3 = (uv.w + pv[3]) - mean[u];
                s[u] += c0 * c0, s[u] += c1 * c1, s[u] += c2 * c2, s[u] += c3 * c3;
            }
        }
#pragma unroll
        for (int u = 0; u < UW; ++u) {
            s[u] += __shfl_xor(s[u], 32, 64);
            rstd[u] = 1.f / sqrtf(s[u] * inv + a.eps);
        }
    }
    // layer 1: K = d inputs formed on the fly, M = d / 2 outputs
    const int K = d, M = d >> 1;
    const float* __restrict__ W = a.w[1];
    f32x16 acc[UW][NB];
    bias_init<UW, NB>(acc, a.b[1], M, h);
    float st[NB * 4];
    chunk_fetch<NB>(st, W, M, K, 0, tid);
    for (int k0 = 0; k0 < K; k0 += NCF_CHUNK) {
        __syncthreads();                                     // every wave is done with the previous chunk
        chunk_store<NB>(st, ws, tid);
        __syncthreads();
        if (k0 + NCF_CHUNK < K) chunk_fetch<NB>(st, W, M, K, k0 + NCF_CHUNK, tid);
        const int kc = min(NCF_CHUNK, K - k0);
        for (int s0 = 0; s0 < kc; s0 += 8)                   // (kc is 16 or 32)
#pragma unroll
        for (int s = s0; s < s0 + 8; s += 2) {
            const int k = s + h;
            const float piv = pi_row[k0 + k], ga = g0_s[k0 + k], be = b0_s[k0 + k];
            float wa[NB];
#pragma unroll
            for (int mb = 0; mb < NB; ++mb) wa[mb] = ws[(mb * 32 + p) * NCF_CHUNK_STRIDE + k];
#pragma unroll
            for (int u = 0; u < UW; ++u) {
                const float hv = relu_keep_nan((((pu_w[u * d + k0 + k] + piv) - mean[u]) * rstd[u]) * ga + be);
#pragma unroll
                for (int mb = 0; mb < NB; ++mb) acc[u][mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[mb], hv, acc[u][mb], 0, 0, 0);
            }
        }
    }
    nms_ln_relu<UW, NB>(acc, a.gamma[1], a.beta[1], M, a.eps, h);
    nms_run_tail<UW, NB>(acc, 2, a, t, ws, tid);
}

// num_layers = 1: logit = predict(relu(LN(Pu[r] + Pi[j]))) (+ GMF), d = factor <= 64; one pair a thread, items on the lanes
__global__ __launch_bounds__(NCF_THREADS) void ncf_model_score_l1_kernel(NmsArgs a) {
    const int64_t j = (int64_t)(blockIdx.x % (unsigned)a.item_tiles) * NCF_THREADS + threadIdx.x;
    const int r = (int)(blockIdx.x / (unsigned)a.item_tiles);
    if (j >= a.n_items || r >= a.n) return;
    const int F = a.factor;
    const bool neumf = a.gu != nullptr;
    const float* wp_mlp = a.wp + (neumf ? F : 0);
    const float* pu = a.pu + (int64_t)r * F;
    const float* pi = a.pi + j * F;
    const float* gamma = a.gamma[0];
    const float* beta = a.beta[0];
    const float inv = 1.f / (float)F;
    float m = 0.f, q = 0.f;
    for (int f = 0; f < F; ++f) m += pu[f] + pi[f];
    m *= inv;
    for (int f = 0; f < F; ++f) {
        const float c = (pu[f] + pi[f]) - m;
        q += c * c;
    }
    const float rstd = 1.f / sqrtf(q * inv + a.eps);
    float s = 0.f;
    for (int f = 0; f < F; ++f) s = fmaf(wp_mlp[f], relu_keep_nan((((pu[f] + pi[f]) - m) * rstd) * gamma[f] + beta[f]), s);
    if (neumf) {
        const int64_t uid = a.users[r];
        if (uid < 0 || uid >= a.user_num) {
            s = __builtin_nanf("");
        } else {
            const float* gu = a.gu + uid * F;
            const float* gi = a.gi + j * F;
            for (int f = 0; f < F; ++f) s = fmaf(a.wp[f], gu[f] * gi[f], s);
        }
    }
    a.scores[(int64_t)r * a.row_stride + j] = s + a.bp[0];
}

// kind GMF: one item a thread with its gi row in registers, NMS_GMF_USERS users a workgroup
template <int F> __global__ __launch_bounds__(NCF_THREADS) void ncf_model_score_gmf_kernel(NmsArgs a) {
    const int64_t j = (int64_t)(blockIdx.x % (unsigned)a.item_tiles) * NCF_THREADS + threadIdx.x;
    const int r0 = (int)(blockIdx.x / (unsigned)a.item_tiles) * NMS_GMF_USERS;
    if (j >= a.n_items) return;
    float gi[F];
#pragma unroll
    for (int f = 0; f < F; ++f) gi[f] = a.gi[j * F + f];
    const float bp = a.bp[0];
    for (int u = 0; u < NMS_GMF_USERS; ++u) {
        const int r = r0 + u;
        if (r >= a.n) break;                                 // (uniform)
        const int64_t uid = a.users[r];
        float s;
        if (uid < 0 || uid >= a.user_num) {                  // (uniform; never read outside the table)
            s = __builtin_nanf("");
        } else {
            const float* gu = a.gu + uid * F;
            float s4[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int f = 0; f < F; ++f) s4[f & 3] = fmaf(a.wp[f], gu[f] * gi[f], s4[f & 3]);
            s = ((s4[0] + s4[1]) + (s4[2] + s4[3])) + bp;
        }
        a.scores[(int64_t)r * a.row_stride + j] = s;
    }
}

template <int UW, int NB> static int nms_launch(const NmsArgs& a, hipStream_t st) {
    const int TU = NCF_WAVES * UW;
    const size_t smem = sizeof(float) * ((size_t)NCF_ITEMS * (a.d + 1) + (size_t)TU * a.d + (size_t)NCF_ITEMS * (a.factor + 1) + (size_t)2 * a.d +
                                         (size_t)32 * NB * NCF_CHUNK_STRIDE);
    const int64_t grid = (int64_t)a.item_tiles * ((a.n + TU - 1) / TU);
    PMGT_CHECK(grid <= 0x7FFFFFFF, -2, "pmgt_ncf_model_score: %lld workgroups exceed the grid limit; split the users", (long long)grid);
    PMGT_SMEM_ATTR(((const void*)ncf_model_score_kernel<UW, NB>), (int)smem);
    hipLaunchKernelGGL((ncf_model_score_kernel<UW, NB>), dim3((unsigned)grid), dim3(NCF_THREADS), smem, st, a);
    return 0;
}

}  // namespace pmgt

using namespace pmgt;

extern "C" int pmgt_ncf_model_score(const pmgt_ncf_model_head* head, const float* pu, const float* pi, const int64_t* users, int64_t n,
                                    int64_t n_items, float* scores, int64_t row_stride, void* stream) {
    const char* who = "pmgt_ncf_model_score";
    PMGT_CHECK(head != nullptr, -2, "%s: NULL head", who);
    const int F = head->factor_num, L = head->num_layers, kind = head->kind;
    PMGT_CHECK(kind == PMGT_NCF_MLP || kind == PMGT_NCF_NEUMF_END || kind == PMGT_NCF_GMF || kind == PMGT_NCF_NEUMF_PRE, -2,
               "%s: unknown model kind %d", who, kind);
    const bool mlp = kind != PMGT_NCF_GMF, gmf = kind != PMGT_NCF_MLP, ln = mlp && head->use_layer_norm != 0;
    int d = 0;
    if (mlp) {
        if (int rc = ncf_head_check(F, L, PMGT_NCF_MLP, who, &d)) return rc;
    } else {
        PMGT_CHECK(F == 8 || F == 16 || F == 32 || F == 64, -2, "%s: factor_num = %d, covered: 8, 16, 32, 64", who, F);
    }
    PMGT_CHECK(std::isfinite(head->layer_norm_eps) && head->layer_norm_eps >= 0.f, -2, "%s: layer_norm_eps = %g is not finite or negative", who,
               (double)head->layer_norm_eps);
    PMGT_CHECK(n >= 1 && n <= PMGT_NCF_MAX_USERS, -2, "%s: n = %lld users outside [1, %d]", who, (long long)n, PMGT_NCF_MAX_USERS);
    PMGT_CHECK(n_items >= 1 && n_items <= 0x7FFFFFFELL, -2, "%s: %lld items outside [1, 2^31 - 2]", who, (long long)n_items);
    PMGT_CHECK(row_stride >= n_items, -2, "%s: row_stride = %lld below the %lld items", who, (long long)row_stride, (long long)n_items);
    PMGT_CHECK(users && scores && head->predict_weight && head->predict_bias && (!mlp || (pu && pi)), -2, "%s: NULL buffer", who);
    if (mlp) {
        for (int i = 1; i < L; ++i) PMGT_CHECK(head->weight[i] && head->bias[i], -2, "%s: NULL parameters of layer %d", who, i);
        if (ln)
            for (int i = 0; i < L; ++i) PMGT_CHECK(head->gamma[i] && head->beta[i], -2, "%s: LayerNorm without gamma / beta of layer %d", who, i);
    }
    PMGT_CHECK(!gmf || (head->gmf_user && head->gmf_item && head->user_num >= 1), -2, "%s: a kind with the GMF branch without its GMF tables", who);
    uintptr_t bits = (uintptr_t)scores | (uintptr_t)head->predict_weight | (uintptr_t)head->predict_bias;
    if (mlp) bits |= (uintptr_t)pu | (uintptr_t)pi;
    if (gmf) bits |= (uintptr_t)head->gmf_user | (uintptr_t)head->gmf_item;
    for (int i = 0; mlp && i < L; ++i) {
        if (i) bits |= (uintptr_t)head->weight[i] | (uintptr_t)head->bias[i];
        if (ln) bits |= (uintptr_t)head->gamma[i] | (uintptr_t)head->beta[i];
    }
    PMGT_CHECK((bits & 3) == 0 && ((uintptr_t)users & 7) == 0, -2, "%s: misaligned buffer", who);
    if (mlp && !ln) {                                        // the head ncf_score.hip scores: its kernels, its bits
        pmgt_ncf_head hd = {};
        hd.factor_num = F, hd.num_layers = L, hd.kind = gmf ? PMGT_NCF_NEUMF_END : PMGT_NCF_MLP;
        for (int i = 1; i < L; ++i) hd.weight[i] = head->weight[i], hd.bias[i] = head->bias[i];
        hd.predict_weight = head->predict_weight, hd.predict_bias = head->predict_bias;
        hd.gmf_user = gmf ? head->gmf_user : nullptr, hd.gmf_item = gmf ? head->gmf_item : nullptr;
        hd.user_num = head->user_num;
        return pmgt_ncf_score(&hd, pu, pi, users, n, n_items, scores, row_stride, stream);
    }
    NmsArgs a = {};
    for (int i = 0; mlp && i < L; ++i) {
        a.w[i] = head->weight[i], a.b[i] = head->bias[i];
        a.gamma[i] = head->gamma[i], a.beta[i] = head->beta[i];
    }
    a.wp = head->predict_weight;
    a.bp = head->predict_bias;
    a.gu = gmf ? head->gmf_user : nullptr;
    a.gi = gmf ? head->gmf_item : nullptr;
    a.pu = pu;
    a.pi = pi;
    a.users = users;
    a.scores = scores;
    a.row_stride = row_stride;
    a.user_num = head->user_num;
    a.eps = head->layer_norm_eps;
    a.n = (int)n;
    a.n_items = (int)n_items;
    a.d = d;
    a.factor = F;
    a.num_layers = mlp ? L : 0;
    hipStream_t st = (hipStream_t)stream;
    if (!mlp) {
        a.item_tiles = (int)((n_items + NCF_THREADS - 1) / NCF_THREADS);
        const int64_t grid = (int64_t)a.item_tiles * ((n + NMS_GMF_USERS - 1) / NMS_GMF_USERS);
        PMGT_CHECK(grid <= 0x7FFFFFFF, -2, "%s: %lld workgroups exceed the grid limit; split the users", who, (long long)grid);
        const dim3 g((unsigned)grid), b(NCF_THREADS);
        if (F == 8) hipLaunchKernelGGL(ncf_model_score_gmf_kernel<8>, g, b, 0, st, a);
        else if (F == 16) hipLaunchKernelGGL(ncf_model_score_gmf_kernel<16>, g, b, 0, st, a);
        else if (F == 32) hipLaunchKernelGGL(ncf_model_score_gmf_kernel<32>, g, b, 0, st, a);
        else hipLaunchKernelGGL(ncf_model_score_gmf_kernel<64>, g, b, 0, st, a);
    } else if (L == 1) {
        a.item_tiles = (int)((n_items + NCF_THREADS - 1) / NCF_THREADS);
        const int64_t grid = (int64_t)a.item_tiles * n;
        PMGT_CHECK(grid <= 0x7FFFFFFF, -2, "%s: %lld workgroups exceed the grid limit; split the users", who, (long long)grid);
        hipLaunchKernelGGL(ncf_model_score_l1_kernel, dim3((unsigned)grid), dim3(NCF_THREADS), 0, st, a);
    } else {
        a.item_tiles = (int)((n_items + NCF_ITEMS - 1) / NCF_ITEMS);
        int rc;
        // blocks of layer 1's output; users per wave: two at the widest layer (128 accumulator registers), four below
        if (d > 128) rc = nms_launch<2, 4>(a, st);
        else if (d > 64) rc = nms_launch<4, 2>(a, st);
        else rc = nms_launch<4, 1>(a, st);
        if (rc) return rc;
    }
    PMGT_LAUNCH_OK();
    return 0;
}
