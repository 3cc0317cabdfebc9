// Fused scoring of a batch of users against the whole catalogue by the eval-mode head of PMGT_NCF (pmgt_ncf_score of include/pmgt_capi.h;
// the head: pmgt/pmgt_ncf/models.py:91-105).  Kept out of csrc/ for eval_metrics.hip's reason: the measured step launches nothing of this.
//
// Layer 0 of the head is linear in the concatenation [user ; item], W0 = [W0u | W0e], so the caller computes once
//       Pu = U_mlp[users] W0u^T   [n, d]         Pi = table W0e^T + b0   [I, d]
// and the kernel forms h1 = relu(Pu[r] + Pi[j]) per pair on the fly, runs layers 1 .. L-1, the optional GMF product and the predict layer,
// and stores ONE float per pair.  fp32 end to end on the exact f32-input MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain).
//
// ORIENTATION.  Every layer is computed TRANSPOSED, Y^T [out, pairs] = W [out, in] H^T [in, pairs]: the A operand is the weight (lane l
// holds W[m = l & 31][k = l >> 5]), the B operand the activations (lane l holds H[pair = l & 31][k = l >> 5]).  A 32 x 32 result block then
// has its PAIR on the lane and its 32 output features in the 16 registers (register g of lane half h = feature (g & 3) + 8 (g >> 2) + 4 h),
// and the next layer sums over exactly that feature index: register g, as it stands, is the B operand of the k-step {rho(g), rho(g) + 4},
// rho(g) = (g & 3) + 8 (g >> 2), the A operand being W[m][32 b + rho(g) + 4 h].  So the activations of a pair never leave the registers of
// its lane between h1 and the logit.  The bias is the accumulator's initial value, the ReLU the only epilogue.  Outputs narrower than 32 are
// zero-padded to one block (weights and biases read as 0 past the true width), so one code path serves factor_num 8 .. 64.
//
// TILE.  A workgroup of 4 waves takes 32 items x 4 UW users; wave w holds the accumulators of users w UW .. w UW + UW - 1 at once, so one
// weight operand read from LDS feeds UW MFMAs per output block.  The Pi rows of the 32 items (row stride d + 1: the column read of a k-step
// is conflict-free), the Pu rows of the users and, for NeuMF-end, the GMF rows of the items sit in LDS.  The weights are STREAMED through one
// LDS buffer in chunks of 32 k-columns ([out][33] floats: 16.5 KiB for the 128 x 256 layer whose 128 KiB would not fit beside the tile); the
// next chunk's global loads are issued before the MFMAs of the current one and stored after them.
// num_layers = 1 has no layer past the split one: relu(Pu + Pi) goes straight into the predict dot product (a VALU kernel, one pair a thread).
// The tile's shape, the chunk transfers, the bias and the predict layer are ncf_score_tile.h's, shared with ncf_model_score.hip.
#include "ncf_score_tile.h"

namespace pmgt {

struct NcfArgs {
    const float* w[NCF_MAX_LAYERS];      // [i]: mlp_layers[i].linear.weight [d >> i][d >> (i - 1)]; [0] is never read (the caller's split)
    const float* b[NCF_MAX_LAYERS];
    const float* wp;                     // predict_layer.weight [factor] or, NeuMF-end, [2 factor] = [gmf | mlp]
    const float* bp;
    const float* gu;                     // gmf_user_embeddings.weight [user_num][factor] or NULL
    const float* gi;                     // gmf_item_embeddings.weight [I][factor] or NULL
    const float* pu;                     // [n][d]
    const float* pi;                     // [I][d]
    const int64_t* users;                // [n]
    float* scores;                       // [n][row_stride]
    int64_t row_stride, user_num;
    int n, n_items, d, factor, num_layers, item_tiles;
};

template <int UW, int NB> __device__ __forceinline__ void relu_all(f32x16 (&acc)[UW][NB]) {
#pragma unroll
    for (int u = 0; u < UW; ++u)
#pragma unroll
        for (int mb = 0; mb < NB; ++mb)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[u][mb][g] = relu_keep_nan(acc[u][mb][g]);
}

// Y = relu(W X + bias) for a layer whose input X sits in the accumulators of the previous one: K true inputs (X is zero past them), M outputs
template <int UW, int NBI, int NBO>
__device__ __forceinline__ void layer_from_acc(const f32x16 (&X)[UW][NBI], f32x16 (&Y)[UW][NBO], const float* __restrict__ W,
                                               const float* __restrict__ bias, int M, int K, float* ws, int tid) {
    const int lane = tid & 63, p = lane & 31, h = lane >> 5;
    bias_init<UW, NBO>(Y, bias, M, h);
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
            float a[NBO];
#pragma unroll
            for (int mb = 0; mb < NBO; ++mb) a[mb] = ws[(mb * 32 + p) * NCF_CHUNK_STRIDE + rho(g) + 4 * h];
#pragma unroll
            for (int u = 0; u < UW; ++u)
#pragma unroll
                for (int mb = 0; mb < NBO; ++mb) Y[u][mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mb], X[u][b][g], Y[u][mb], 0, 0, 0);
        }
    }
    relu_all<UW, NBO>(Y);
}

// the layers behind `layer - 1`, halving the block count while it is above one, then the predict layer
template <int UW, int NBI>
__device__ __forceinline__ void run_tail(f32x16 (&X)[UW][NBI], int layer, const NcfArgs& a, const NcfTile& t, float* ws, int tid) {
    if constexpr (NBI > 1) {
        if (layer < a.num_layers) {
            f32x16 Y[UW][NBI / 2];
            layer_from_acc<UW, NBI, NBI / 2>(X, Y, a.w[layer], a.b[layer], a.d >> layer, a.d >> (layer - 1), ws, tid);
            run_tail<UW, NBI / 2>(Y, layer + 1, a, t, ws, tid);
        } else {
            predict_store<UW, NBI>(X, a, t);
        }
    } else {
        for (; layer < a.num_layers; ++layer) {
            f32x16 Y[UW][1];
            layer_from_acc<UW, 1, 1>(X, Y, a.w[layer], a.b[layer], a.d >> layer, a.d >> (layer - 1), ws, tid);
#pragma unroll
            for (int u = 0; u < UW; ++u) X[u][0] = Y[u][0];
        }
        predict_store<UW, 1>(X, a, t);
    }
}

// NB = 32-row blocks of layer 1's output (d / 2 rounded up to 32); dynamic LDS: Pi tile | Pu tile | GMF item tile | weight chunk
template <int UW, int NB> __global__ __launch_bounds__(NCF_THREADS) void ncf_score_kernel(NcfArgs a) {
    extern __shared__ float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = lane & 31, h = lane >> 5;
    const int d = a.d, F = a.factor, TU = NCF_WAVES * UW;
    float* pi_s = smem;                                      // [32][d + 1]
    float* pu_s = pi_s + NCF_ITEMS * (d + 1);                // [TU][d]
    float* gi_s = pu_s + TU * d;                             // [32][F + 1]
    float* ws = gi_s + NCF_ITEMS * (F + 1);                  // [32 NB][33]
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
    // layer 1: K = d inputs formed on the fly, M = d / 2 outputs
    const int K = d, M = d >> 1;
    const float* __restrict__ W = a.w[1];
    f32x16 acc[UW][NB];
    bias_init<UW, NB>(acc, a.b[1], M, h);
    float st[NB * 4];
    chunk_fetch<NB>(st, W, M, K, 0, tid);
    const float* pu_w = pu_s + wave * UW * d;
    for (int k0 = 0; k0 < K; k0 += NCF_CHUNK) {
        __syncthreads();                                     // the tiles are written / every wave is done with the previous chunk
        chunk_store<NB>(st, ws, tid);
        __syncthreads();
        if (k0 + NCF_CHUNK < K) chunk_fetch<NB>(st, W, M, K, k0 + NCF_CHUNK, tid);
        const int kc = min(NCF_CHUNK, K - k0);
        for (int s0 = 0; s0 < kc; s0 += 8)                   // (kc is 16 or 32)
#pragma unroll
        for (int s = s0; s < s0 + 8; s += 2) {
            const int k = s + h;
            const float piv = pi_s[p * (d + 1) + k0 + k];
            float wa[NB];
#pragma unroll
            for (int mb = 0; mb < NB; ++mb) wa[mb] = ws[(mb * 32 + p) * NCF_CHUNK_STRIDE + k];
#pragma unroll
            for (int u = 0; u < UW; ++u) {
                const float hv = relu_keep_nan(pu_w[u * d + k0 + k] + piv);
#pragma unroll
                for (int mb = 0; mb < NB; ++mb) acc[u][mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[mb], hv, acc[u][mb], 0, 0, 0);
            }
        }
    }
    relu_all<UW, NB>(acc);
    run_tail<UW, NB>(acc, 2, a, t, ws, tid);
}

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

template <int UW, int NB> static int ncf_launch(const NcfArgs& a, hipStream_t st) {
    const int TU = NCF_WAVES * UW;
    const size_t smem = sizeof(float) * ((size_t)NCF_ITEMS * (a.d + 1) + (size_t)TU * a.d + (size_t)NCF_ITEMS * (a.factor + 1) +
                                         (size_t)32 * NB * NCF_CHUNK_STRIDE);
    const int64_t grid = (int64_t)a.item_tiles * ((a.n + TU - 1) / TU);
    PMGT_CHECK(grid <= 0x7FFFFFFF, -2, "pmgt_ncf_score: %lld workgroups exceed the grid limit; split the users", (long long)grid);
    PMGT_SMEM_ATTR(((const void*)ncf_score_kernel<UW, NB>), (int)smem);
    hipLaunchKernelGGL((ncf_score_kernel<UW, NB>), dim3((unsigned)grid), dim3(NCF_THREADS), smem, st, a);
    return 0;
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
    NcfArgs a;
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
    } else {
        a.item_tiles = (int)((n_items + NCF_ITEMS - 1) / NCF_ITEMS);
        int rc;
        // blocks of layer 1's output; users per wave: two at the widest layer (128 accumulator registers), four below
        if (d > 128) rc = ncf_launch<2, 4>(a, st);
        else if (d > 64) rc = ncf_launch<4, 2>(a, st);
        else rc = ncf_launch<4, 1>(a, st);
        if (rc) return rc;
    }
    PMGT_LAUNCH_OK();
    return 0;
}
