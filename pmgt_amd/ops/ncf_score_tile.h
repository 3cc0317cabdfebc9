// The MLP scoring tower of the three whole-catalogue scorers, stated once: ncf_score.hip (the head of PMGT_NCF: LN = false),
// ncf_model_score.hip (the stand-alone NCF class with LayerNorm: LN = true) and dcn_score.hip (the deep net of the DCN, both).  fp32 end to
// end on the exact f32-input MFMA (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain), no atomic, ONE float stored per pair.
//
// Layer 0 of the tower is linear in the concatenation [user ; item], W0 = [W0u | W0e], so the caller computes once
//       Pu = U[users] W0u^T   [n, d]         Pi = table W0e^T + b0   [I, d]
// and the kernel forms h1 = relu([LN_0](Pu[r] + Pi[j])) per pair on the fly, runs the layers 1 .. L-1 (Linear -> [LayerNorm ->] ReLU, the
// widths halving from d), and hands the last activations to the file's final store (predict_store below, or the DCN's output layer).
//
// ORIENTATION.  Every layer is computed TRANSPOSED, Y^T [out, pairs] = W [out, in] H^T [in, pairs]: the A operand is the weight (lane l
// holds W[m = l & 31][k = l >> 5]), the B operand the activations (lane l holds H[pair = l & 31][k = l >> 5]).  A 32 x 32 result block then
// has its PAIR on the lane and its 32 output features in the 16 registers (register g of lane half h = feature (g & 3) + 8 (g >> 2) + 4 h),
// and the next layer sums over exactly that feature index: register g, as it stands, is the B operand of the k-step {rho(g), rho(g) + 4},
// rho(g) = (g & 3) + 8 (g >> 2), the A operand being W[m][32 b + rho(g) + 4 h].  So the activations of a pair never leave the registers of
// its lane between h1 and the logit.  The bias is the accumulator's initial value.  Outputs narrower than 32 are zero-padded to one block
// (weights and biases read as 0 past the true width), so one code path serves every width.
//
// TILE.  A workgroup of 4 waves takes 32 items x 4 UW users; wave w holds the accumulators of users w UW .. w UW + UW - 1 at once, so one
// weight operand read from LDS feeds UW MFMAs per output block.  The Pi rows of the 32 items (row stride d + 1: the column read of a k-step
// is conflict-free), the Pu rows of the users and the file's own tiles sit in LDS.  The weights are STREAMED through one LDS buffer in
// chunks of 32 k-columns ([out][33] floats: 16.5 KiB for the 128 x 256 layer whose 128 KiB would not fit beside the tile); the next
// chunk's global loads are issued before the MFMAs of the current one and stored after them.  <UW, NB> by d: <2, 4> above 128 (128
// accumulator registers), <4, 2> above 64, <4, 1> below; NB = the 32-row blocks of layer 1's output.
//
// LAYERNORM (LN = true).  Layer 0: before the k-loop every lane computes its pair's mean and rstd over the d features of y = Pu[r] + Pi[j]:
// lane half h sums the features [h d / 2, (h + 1) d / 2) in order, the halves exchange once (a + b and b + a are the same float, so both
// halves hold the same bits), then the same for the squared deviations; the k-loop feeds relu(((y - mean) rstd) gamma0[k] + beta0[k]),
// gamma0 / beta0 in LDS.  Layer l: the M = d >> l outputs of a pair sit in the 16 registers x NB blocks of its lane and of lane ^ 32: a
// register sum plus one exchange, before the ReLU; features past M take no part, the divisor is M, and they are written back as 0.  Two
// passes, biased variance, rstd = 1 / sqrt(var + eps), ONE accumulation chain per product (K <= 256).
// CONTRACTION.  The LayerNorm arithmetic must not be fused into fmas (q * inv + eps, (x - mean) * rstd * ga + be: the bits are pinned by
// tests/golden/score_tower_bits.json).  That does not rest on the including file: every block below that holds such an expression opens
// with `#pragma clang fp contract(off)`, which clang records in the expressions when the template is PARSED, so each instance has it
// whatever the includer's setting.  (ncf_model_score.hip and dcn_score.hip also set it for their whole file; ncf_score.hip does not.)
//
// NaN.  A pair's values live on the two lanes of its item only (the MFMA's B column, the one exchange with lane ^ 32), and the ReLU keeps a
// NaN: a NaN in a row of Pi reaches every score of that item and no other.
//
// Every function is inlined into its caller.  Args is the caller's argument struct, read by name: w, b, gamma, beta, eps (fields of every
// Args, dereferenced with LN only), pu, pi, d, num_layers, n, n_items, item_tiles by the tower; wp, bp, gu, users, scores, row_stride,
// user_num, factor by predict_store.
#pragma once
#include "ncf_head.h"

namespace pmgt {

static constexpr int NCF_THREADS = 256, NCF_WAVES = 4, NCF_ITEMS = 32;      // one workgroup: 4 waves, 32 items
static constexpr int NCF_CHUNK = 32, NCF_CHUNK_STRIDE = NCF_CHUNK + 1;      // k-columns of one weight chunk, its LDS row stride
static constexpr int NCF_MAX_LAYERS = PMGT_NCF_MAX_LAYERS;

// rows [0, 32 NBO) x k-columns [k0, k0 + 32) of W [M][K], zero past M and K: global -> registers, registers -> LDS [m][33]
template <int NBO> __device__ __forceinline__ void chunk_fetch(float (&st)[NBO * 4], const float* __restrict__ W, int M, int K, int k0, int tid) {
#pragma unroll
    for (int i = 0; i < NBO * 4; ++i) {
        const int e = tid + NCF_THREADS * i, c = e & 31, m = e >> 5;
        st[i] = (m < M && k0 + c < K) ? W[(int64_t)m * K + k0 + c] : 0.f;
    }
}
template <int NBO> __device__ __forceinline__ void chunk_store(const float (&st)[NBO * 4], float* ws, int tid) {
#pragma unroll
    for (int i = 0; i < NBO * 4; ++i) {
        const int e = tid + NCF_THREADS * i, c = e & 31, m = e >> 5;
        ws[m * NCF_CHUNK_STRIDE + c] = st[i];
    }
}
// the accumulators of a layer start as its bias: feature 32 mb + rho(g) + 4 h in register g
template <int UW, int NBO> __device__ __forceinline__ void bias_init(f32x16 (&acc)[UW][NBO], const float* __restrict__ bias, int M, int h) {
#pragma unroll
    for (int mb = 0; mb < NBO; ++mb)
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int f = mb * 32 + rho(g) + 4 * h;
            const float v = f < M ? bias[f] : 0.f;
#pragma unroll
            for (int u = 0; u < UW; ++u) acc[u][mb][g] = v;
        }
}

// the dynamic LDS of a tower kernel, in floats: Pi tile [32][d + 1] | Pu tile [TU][d] | the file's own tiles [own] | gamma0, beta0 [d]
// each (norm0) | weight chunk [32 NB][33]
struct TowerLds {
    float *pi_s, *pu_s, *own, *g0_s, *b0_s, *ws;
};
__host__ __device__ __forceinline__ size_t tower_lds_floats(int d, int TU, int NB, int own, bool norm0) {
    return (size_t)NCF_ITEMS * (d + 1) + (size_t)TU * d + (size_t)own + (norm0 ? (size_t)2 * d : 0) + (size_t)32 * NB * NCF_CHUNK_STRIDE;
}
__device__ __forceinline__ TowerLds tower_lds(float* smem, int d, int TU, int own, bool norm0) {
    TowerLds s;
    s.pi_s = smem;
    s.pu_s = s.pi_s + NCF_ITEMS * (d + 1);
    s.own = s.pu_s + TU * d;
    s.g0_s = s.own + own;
    s.b0_s = s.g0_s + (norm0 ? d : 0);
    s.ws = s.b0_s + (norm0 ? d : 0);
    return s;
}

// the Pi rows of the items j0 .. j0 + 31, the Pu rows of the users r0 .. r0 + 4 UW - 1 and, with LayerNorm, gamma0 / beta0 -> LDS; rows
// outside the batch / the catalogue are zeros: computed, never stored
template <bool LN, int UW, class Args> __device__ __forceinline__ void tower_load_tiles(const Args& a, const TowerLds& s, int r0, int j0, int tid) {
    const int d = a.d, TU = NCF_WAVES * UW;
    for (int e = tid; e < NCF_ITEMS * d; e += NCF_THREADS) {
        const int row = e / d, c = e - row * d, j = j0 + row;
        s.pi_s[row * (d + 1) + c] = j < a.n_items ? a.pi[(int64_t)j * d + c] : 0.f;
    }
    for (int e = tid; e < TU * d; e += NCF_THREADS) {
        const int row = e / d, c = e - row * d, r = r0 + row;
        s.pu_s[e] = r < a.n ? a.pu[(int64_t)r * d + c] : 0.f;
    }
    if constexpr (LN)
        for (int e = tid; e < d; e += NCF_THREADS) s.g0_s[e] = a.gamma[0][e], s.b0_s[e] = a.beta[0][e];
}

// the statistics of layer 0's row y = Pu[r] + Pi[j] of every pair of the lane (the tiles are written and a barrier has passed): each lane
// half sums its half of the features, one exchange.  pu_w: the wave's Pu rows in LDS; pi_row: the lane's Pi row
template <int UW>
__device__ __forceinline__ void tower_row_stats(const float* pu_w, const float* pi_row, int d, float eps, int h, float (&mean)[UW], float (&rstd)[UW]) {
#pragma clang fp contract(off)
    const int half = d >> 1, f0 = h * half;
    const float inv = 1.f / (float)d;                        // (d is a power of two)
    float s[UW];
#pragma unroll
    for (int u = 0; u < UW; ++u) s[u] = 0.f;
    for (int k = f0; k < f0 + half; k += 4) {                // (half is a multiple of 8; the Pu rows are 16-byte aligned in LDS)
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
        rstd[u] = 1.f / sqrtf(s[u] * inv + eps);
    }
}

// acc = relu(acc) or, LN, relu(LN(acc)) over the M true features of every pair (feature 32 mb + rho(g) + 4 h of pair p in acc[u][mb][g],
// the other half of the features on lane ^ 32); with LN the features past M come out as 0
template <bool LN, int UW, int NB>
__device__ __forceinline__ void tower_norm_relu(f32x16 (&acc)[UW][NB], const float* __restrict__ gamma, const float* __restrict__ beta, int M, float eps,
                                                int h) {
    if constexpr (!LN) {
#pragma unroll
        for (int u = 0; u < UW; ++u)
#pragma unroll
            for (int mb = 0; mb < NB; ++mb)
#pragma unroll
                for (int g = 0; g < 16; ++g) acc[u][mb][g] = relu_keep_nan(acc[u][mb][g]);
    } else {
#pragma clang fp contract(off)
        const float inv = 1.f / (float)M;                    // (M is a power of two: the product is the quotient)
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
}

// layer 1: acc = relu([LN](W_1 h1 + b_1)) with the K = d inputs h1 = relu([LN_0](Pu[r] + Pi[j])) formed on the fly from the LDS tiles (mean,
// rstd: tower_row_stats', read with LN only), M = d / 2 outputs.  The first barrier of the k-loop also covers the tile writes
template <bool LN, int UW, int NB, class Args>
__device__ __forceinline__ void tower_first_layer(f32x16 (&acc)[UW][NB], const Args& a, const TowerLds& s, const float* pu_w, const float* pi_row,
                                                  const float (&mean)[UW], const float (&rstd)[UW], int tid) {
    const int lane = tid & 63, p = lane & 31, h = lane >> 5;
    const int d = a.d, K = d, M = d >> 1;
    const float* __restrict__ W = a.w[1];
    float* ws = s.ws;
    bias_init<UW, NB>(acc, a.b[1], M, h);
    float st[NB * 4];
    chunk_fetch<NB>(st, W, M, K, 0, tid);
    for (int k0 = 0; k0 < K; k0 += NCF_CHUNK) {
        __syncthreads();                                     // the tiles are written / every wave is done with the previous chunk
        chunk_store<NB>(st, ws, tid);
        __syncthreads();
        if (k0 + NCF_CHUNK < K) chunk_fetch<NB>(st, W, M, K, k0 + NCF_CHUNK, tid);
        const int kc = min(NCF_CHUNK, K - k0);
        for (int s0 = 0; s0 < kc; s0 += 8)                   // (kc is 16 or 32)
#pragma unroll
        for (int sk = s0; sk < s0 + 8; sk += 2) {
            const int k = sk + h;
            const float piv = pi_row[k0 + k];
            float ga = 0.f, be = 0.f;
            if constexpr (LN) ga = s.g0_s[k0 + k], be = s.b0_s[k0 + k];
            float wa[NB];
#pragma unroll
            for (int mb = 0; mb < NB; ++mb) wa[mb] = ws[(mb * 32 + p) * NCF_CHUNK_STRIDE + k];
#pragma unroll
            for (int u = 0; u < UW; ++u) {
                float hv = pu_w[u * d + k0 + k] + piv;
                if constexpr (LN) {
#pragma clang fp contract(off)
                    hv = ((hv - mean[u]) * rstd[u]) * ga + be;
                }
                hv = relu_keep_nan(hv);
#pragma unroll
                for (int mb = 0; mb < NB; ++mb) acc[u][mb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[mb], hv, acc[u][mb], 0, 0, 0);
            }
        }
    }
    tower_norm_relu<LN, UW, NB>(acc, a.gamma[1], a.beta[1], M, a.eps, h);
}

// Y = relu([LN](W X + bias)) for layer `layer` >= 2, whose input X sits in the accumulators of the previous one: K = d >> (layer - 1) true
// inputs (X is zero past them), M = d >> layer outputs
template <bool LN, int UW, int NBI, int NBO, class Args>
__device__ __forceinline__ void tower_layer_from_acc(const f32x16 (&X)[UW][NBI], f32x16 (&Y)[UW][NBO], const Args& a, int layer, float* ws, int tid) {
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
    tower_norm_relu<LN, UW, NBO>(Y, a.gamma[layer], a.beta[layer], M, a.eps, h);
}

// the layers behind `layer - 1`, halving the block count while it is above one, then the file's final store: store(X) for the last
// activations X [UW][blocks] (a generic callable: the block count is only known here)
template <bool LN, int UW, int NBI, class Args, class Store>
__device__ __forceinline__ void tower_run_tail(f32x16 (&X)[UW][NBI], int layer, const Args& a, float* ws, int tid, const Store& store) {
    if constexpr (NBI > 1) {
        if (layer < a.num_layers) {
            f32x16 Y[UW][NBI / 2];
            tower_layer_from_acc<LN, UW, NBI, NBI / 2>(X, Y, a, layer, ws, tid);
            tower_run_tail<LN, UW, NBI / 2>(Y, layer + 1, a, ws, tid, store);
        } else {
            store(X);
        }
    } else {
        for (; layer < a.num_layers; ++layer) {
            f32x16 Y[UW][1];
            tower_layer_from_acc<LN, UW, 1, 1>(X, Y, a, layer, ws, tid);
#pragma unroll
            for (int u = 0; u < UW; ++u) X[u][0] = Y[u][0];
        }
        store(X);
    }
}

// one launch of a tower kernel over a.item_tiles x ceil(n / TU) workgroups; attr_bytes: what the kernel is allowed of dynamic LDS (set once
// per kernel and device); refuses a grid past the limit in the name of the entry `who`
template <class Args, void (*Kernel)(Args)>
int tower_launch(const char* who, const Args& a, int TU, size_t smem_bytes, int attr_bytes, hipStream_t st) {
    const int64_t grid = (int64_t)a.item_tiles * ((a.n + TU - 1) / TU);
    PMGT_CHECK(grid <= 0x7FFFFFFF, -2, "%s: %lld workgroups exceed the grid limit; split the users", who, (long long)grid);
    PMGT_SMEM_ATTR(((const void*)Kernel), attr_bytes);
    hipLaunchKernelGGL(Kernel, dim3((unsigned)grid), dim3(NCF_THREADS), smem_bytes, st, a);
    return 0;
}

// ---- the two NCF files: one argument struct, the GMF item tile, the predict layer, one tile kernel ---------------------------------------
struct NcfArgs {
    const float* w[NCF_MAX_LAYERS];      // [i]: W_i [d >> i][d >> (i - 1)]; [0] is never read (the caller's split)
    const float* b[NCF_MAX_LAYERS];
    const float* gamma[NCF_MAX_LAYERS];  // LayerNorm of layer i over d >> i features (ncf_model_score.hip; else unread)
    const float* beta[NCF_MAX_LAYERS];
    const float* wp;                     // predict_layer.weight [factor] or, with both branches, [2 factor] = [gmf | mlp]
    const float* bp;
    const float* gu;                     // the GMF user table [user_num][factor] or NULL
    const float* gi;                     // the GMF item table [I][factor] or NULL
    const float* pu;                     // [n][d]
    const float* pi;                     // [I][d]
    const int64_t* users;                // [n]
    float* scores;                       // [n][row_stride]
    int64_t row_stride, user_num;
    float eps;
    int n, n_items, d, factor, num_layers, item_tiles;
};

struct NcfTile {
    const float* gi_s;      // LDS [32][factor + 1] or unused
    int r0, j0, wave, lane;
};

// the predict layer on the last activations (features 32 b + rho(g) + 4 h of pair p in X[u][b][g]) plus the GMF branch; one store per pair
template <int UW, int NB, class Args> __device__ __forceinline__ void predict_store(const f32x16 (&X)[UW][NB], const Args& a, const NcfTile& t) {
    const int p = t.lane & 31, h = t.lane >> 5, F = a.factor;
    const bool neumf = a.gu != nullptr;
    const float* wp_mlp = a.wp + (neumf ? F : 0);
    const float bp = a.bp[0];
#pragma unroll
    for (int u = 0; u < UW; ++u) {
        const int r = t.r0 + t.wave * UW + u;
        float s = 0.f;
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int f = b * 32 + rho(g) + 4 * h;
                if (f < F) s = fmaf(wp_mlp[f], X[u][b][g], s);
            }
        bool bad_user = false;
        if (neumf && r < a.n) {                      // (uniform per wave)
            const int64_t uid = a.users[r];
            bad_user = uid < 0 || uid >= a.user_num;
            if (!bad_user) {
                const float* gu = a.gu + uid * F;
                const int half = F >> 1;             // F >= 8: each lane half takes half of the factors
                for (int f = h * half; f < (h + 1) * half; ++f) s = fmaf(a.wp[f], gu[f] * t.gi_s[p * (F + 1) + f], s);
            }
        }
        s += __shfl_xor(s, 32, 64);
        s += bp;
        if (bad_user) s = __builtin_nanf("");        // (the host surface refuses such ids; never read outside the table)
        const int j = t.j0 + p;
        if (h == 0 && r < a.n && j < a.n_items) a.scores[(int64_t)r * a.row_stride + j] = s;
    }
}

// num_layers >= 2 of both NCF files.  The file's own LDS tile is the GMF rows of the 32 items [32][factor + 1]; gamma0 / beta0 are
// reserved with LN only
template <bool LN, int UW, int NB> __global__ __launch_bounds__(NCF_THREADS) void ncf_tile_kernel(NcfArgs a) {
    extern __shared__ __align__(16) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = lane & 31, h = lane >> 5;
    const int d = a.d, F = a.factor, TU = NCF_WAVES * UW;
    const TowerLds s = tower_lds(smem, d, TU, NCF_ITEMS * (F + 1), LN);
    float* gi_s = s.own;
    NcfTile t;
    t.j0 = (int)(blockIdx.x % (unsigned)a.item_tiles) * NCF_ITEMS;
    t.r0 = (int)(blockIdx.x / (unsigned)a.item_tiles) * TU;
    t.wave = wave;
    t.lane = lane;
    t.gi_s = gi_s;
    tower_load_tiles<LN, UW>(a, s, t.r0, t.j0, tid);
    if (a.gi)
        for (int e = tid; e < NCF_ITEMS * F; e += NCF_THREADS) {
            const int row = e / F, c = e - row * F, j = t.j0 + row;
            gi_s[row * (F + 1) + c] = j < a.n_items ? a.gi[(int64_t)j * F + c] : 0.f;
        }
    const float* pu_w = s.pu_s + wave * UW * d;
    const float* pi_row = s.pi_s + p * (d + 1);
    float mean[UW], rstd[UW];
    if constexpr (LN) {
        __syncthreads();                                     // the tiles are written
        tower_row_stats<UW>(pu_w, pi_row, d, a.eps, h, mean, rstd);
    }
    f32x16 acc[UW][NB];
    tower_first_layer<LN, UW, NB>(acc, a, s, pu_w, pi_row, mean, rstd, tid);
    tower_run_tail<LN, UW, NB>(acc, 2, a, s.ws, tid, [&](const auto& X) { predict_store(X, a, t); });
}

template <bool LN, int UW, int NB> int ncf_tile_launch_as(const char* who, const NcfArgs& a, hipStream_t st) {
    const int TU = NCF_WAVES * UW;
    const size_t smem = sizeof(float) * tower_lds_floats(a.d, TU, NB, NCF_ITEMS * (a.factor + 1), LN);
    return tower_launch<NcfArgs, ncf_tile_kernel<LN, UW, NB>>(who, a, TU, smem, (int)smem, st);
}
// a.item_tiles is set here
template <bool LN> int ncf_tile_launch(const char* who, NcfArgs& a, hipStream_t st) {
    a.item_tiles = (int)(((int64_t)a.n_items + NCF_ITEMS - 1) / NCF_ITEMS);
    if (a.d > 128) return ncf_tile_launch_as<LN, 2, 4>(who, a, st);
    if (a.d > 64) return ncf_tile_launch_as<LN, 4, 2>(who, a, st);
    return ncf_tile_launch_as<LN, 4, 1>(who, a, st);
}

}  // namespace pmgt
