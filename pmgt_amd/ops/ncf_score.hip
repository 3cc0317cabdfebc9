// Fused scoring of a batch of users against the whole catalogue by the eval-mode head of PMGT_NCF (pmgt_ncf_score of include/pmgt_capi.h;
// the head: pmgt/pmgt_ncf/models.py:91-105).  Kept out of csrc/ for eval_metrics.hip's reason: the measured step launches nothing of this.
//
// The MLP tower -- layer 0 split into Pu and Pi by the caller, every layer transposed on the 32x32x2 f32 MFMA, the activations of a pair chained
// in the registers of its lane, the weights streamed through LDS, the tile, the argument struct and the predict layer with the GMF branch -- is
// ncf_score_tile.h's, whose header states the design; this head has no LayerNorm, so the tile kernel here is its LN = false instance, and
// the file is compiled with the default contraction (the tower multiplies only inside the MFMA and explicit fmaf).
// num_layers = 1 has no layer past the split one: relu(Pu + Pi) goes straight into the predict dot product (a VALU kernel, one pair a thread).
#include "ncf_score_tile.h"

namespace pmgt {

// num_layers = 1: logit = predict(relu(Pu[r] + Pi[j])) (+ GMF), d = factor <= 64; one pair a thread, items on the lanes
__global__ __launch_bounds__(NCF_THREADS) void ncf_score_l1_kernel(NcfArgs a) {
    const int64_t j = (int64_t)(blockIdx.x % (unsigned)a.item_tiles) * NCF_THREADS + threadIdx.x;
    const int r = (int)(blockIdx.x / (unsigned)a.item_tiles);
    if (j >= a.n_items || r >= a.n) return;
    const int F = a.factor;
    const bool neumf = a.gu != nullptr;
    const float* wp_mlp = a.wp + (neumf ? F : 0);
    const float* pu = a.pu + (int64_t)r * F;
    const float* pi = a.pi + j * F;
    float s = 0.f;
    for (int f = 0; f < F; ++f) s = fmaf(wp_mlp[f], relu_keep_nan(pu[f] + pi[f]), s);
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

}  // namespace pmgt

using namespace pmgt;

extern "C" int pmgt_ncf_score(const pmgt_ncf_head* head, const float* pu, const float* pi, const int64_t* users, int64_t n, int64_t n_items,
                              float* scores, int64_t row_stride, void* stream) {
    PMGT_CHECK(head != nullptr, -2, "pmgt_ncf_score: NULL head");
    const int F = head->factor_num, L = head->num_layers;
    int d;
    if (int rc = ncf_head_check(F, L, head->kind, "pmgt_ncf_score", &d)) return rc;
    const bool neumf = head->kind == PMGT_NCF_NEUMF_END;
    PMGT_CHECK(n >= 1 && n <= PMGT_NCF_MAX_USERS, -2, "pmgt_ncf_score: n = %lld users outside [1, %d]", (long long)n, PMGT_NCF_MAX_USERS);
    PMGT_CHECK(n_items >= 1 && n_items <= 0x7FFFFFFELL, -2, "pmgt_ncf_score: %lld items outside [1, 2^31 - 2]", (long long)n_items);
    PMGT_CHECK(row_stride >= n_items, -2, "pmgt_ncf_score: row_stride = %lld below the %lld items", (long long)row_stride, (long long)n_items);
    PMGT_CHECK(pu && pi && users && scores && head->predict_weight && head->predict_bias, -2, "pmgt_ncf_score: NULL buffer");
    for (int i = 1; i < L; ++i) PMGT_CHECK(head->weight[i] && head->bias[i], -2, "pmgt_ncf_score: NULL parameters of layer %d", i);
    PMGT_CHECK(!neumf || (head->gmf_user && head->gmf_item && head->user_num >= 1), -2, "pmgt_ncf_score: NeuMF-end without its GMF tables");
    PMGT_CHECK((((uintptr_t)pu | (uintptr_t)pi | (uintptr_t)scores) & 3) == 0 && ((uintptr_t)users & 7) == 0, -2,
               "pmgt_ncf_score: misaligned buffer");
    NcfArgs a = {};
    for (int i = 0; i < NCF_MAX_LAYERS; ++i) {
        a.w[i] = i < L ? head->weight[i] : nullptr;
        a.b[i] = i < L ? head->bias[i] : nullptr;
    }
    a.wp = head->predict_weight;
    a.bp = head->predict_bias;
    a.gu = neumf ? head->gmf_user : nullptr;
    a.gi = neumf ? head->gmf_item : nullptr;
    a.pu = pu;
    a.pi = pi;
    a.users = users;
    a.scores = scores;
    a.row_stride = row_stride;
    a.user_num = head->user_num;
    a.n = (int)n;
    a.n_items = (int)n_items;
    a.d = d;
    a.factor = F;
    a.num_layers = L;
    hipStream_t st = (hipStream_t)stream;
    if (L == 1) {
        a.item_tiles = (int)((n_items + NCF_THREADS - 1) / NCF_THREADS);
        const int64_t grid = (int64_t)a.item_tiles * n;
        PMGT_CHECK(grid <= 0x7FFFFFFF, -2, "pmgt_ncf_score: %lld workgroups exceed the grid limit; split the users", (long long)grid);
        hipLaunchKernelGGL(ncf_score_l1_kernel, dim3((unsigned)grid), dim3(NCF_THREADS), 0, st, a);
    } else if (int rc = ncf_tile_launch<false>("pmgt_ncf_score", a, st)) {
        return rc;
    }
    PMGT_LAUNCH_OK();
    return 0;
}
