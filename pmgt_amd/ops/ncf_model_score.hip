// Fused scoring of a batch of users against the whole catalogue by the eval-mode head of the reference's stand-alone NCF class
// (pmgt_ncf_model_score of include/pmgt_capi.h; the class: pmgt/ncf/models.py:14-154, restated in pmgt_amd/ncf.py).  Kept out of csrc/ for
// eval_metrics.hip's reason.  fp32 end to end, no atomic, one float stored per pair, the same bits for the same inputs.
//
// WHICH CASES RUN HERE.  A model WITHOUT LayerNorm of kind MLP / NeuMF-end / NeuMF-pre is the head ncf_score.hip scores: the entry hands it
// to pmgt_ncf_score, so those bits are that file's.  The kernels below cover the LayerNorm layer  h_(l+1) = relu(LN_l(W_l h_l + b_l))  and
// kind GMF.  The MLP tower, its LayerNorm (layer 0's row statistics from the LDS tiles, layer l's from the registers; the numerics are
// ncf_model_train.hip's: two passes, biased variance, rstd = 1 / sqrt(var + eps), no contraction) and the tile kernel are
// ncf_score_tile.h's, whose header states the design: the tile kernel here is its LN = true instance.  The products keep ONE accumulation
// chain: K is at most 256 here (ncf_model_train.hip's K = 512 needed four): the k-ordered chain emulated on the host stays within 1.5 x the
// fp32 formula's error at d = 256, dealing the steps onto two or four accumulators gains nothing there, and the device gives 1.62 x at most
// (the bound is 4 x).
//   L = 1.     One pair a thread (ncf_score.hip's VALU kernel) with the LayerNorm over the F features in front of the predict dot.
//   GMF.       scores[r][j] = sum_f wp[f] (gu[users[r]][f] gi[j][f]) + bp: one item a thread, its gi row in registers, 8 users a workgroup
//              (their gu rows are uniform loads), the dot dealt onto four sums joined as (a + b) + (c + d).  No MLP tensor is read.
#include <cmath>

#pragma clang fp contract(off)

#include "ncf_score_tile.h"

namespace pmgt {

static constexpr int NMS_GMF_USERS = 8;                                     // users a workgroup of the GMF kernel

// num_layers = 1: logit = predict(relu(LN(Pu[r] + Pi[j]))) (+ GMF), d = factor <= 64; one pair a thread, items on the lanes
__global__ __launch_bounds__(NCF_THREADS) void ncf_model_score_l1_kernel(NcfArgs a) {
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
template <int F> __global__ __launch_bounds__(NCF_THREADS) void ncf_model_score_gmf_kernel(NcfArgs a) {
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
    NcfArgs a = {};
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
    } else if (int rc = ncf_tile_launch<true>(who, a, st)) {
        return rc;
    }
    PMGT_LAUNCH_OK();
    return 0;
}
