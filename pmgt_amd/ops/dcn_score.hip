// Fused scoring of a batch of users against the whole catalogue by the eval-mode Deep & Cross Network (pmgt_dcn_score_rows and
// pmgt_dcn_score of include/pmgt_capi.h; the model: pmgt/dcn/models.py, restated in pmgt_amd/dcn_head.py).  Kept out of csrc/ for
// eval_metrics.hip's reason: the measured step launches nothing of this.  fp32 end to end, compiled without contraction, no atomic, one
// float stored per pair, the same bits for the same inputs.
//
// THE DEEP NET is the NCF MLP tower with factor' = 2 F, layers' = L, d' = E: every layer is Linear -> LayerNorm -> ReLU (or Linear -> ReLU),
// the widths run 2 E -> E -> ... -> 2 F, and layer 0 splits into a per-user and a per-item half that the caller computes (Pu [n][E],
// Pi [I][E] with b_0 folded in).  The tower, with and without LayerNorm, is ncf_score_tile.h's, whose header states the design; this file
// adds the row scalars in LDS and the output layer with the cross net as the tower's final store.  The last deep width is 2 F, up to 128:
// four 32-feature blocks in the output dot.
//
// THE CROSS NET COLLAPSES (dcn_head.py's header): the reference's layer adds x0, not x^(c), so every cross state is a scalar multiple of x0
// (no LayerNorm) or an affine image of the centred x0 (LayerNorm), and every s_c and the output dot split into one scalar per user row plus
// one per item row.  pmgt_dcn_score_rows writes those scalars (mu, q, d_0 .. d_C; one wave a row, the elements lane, lane + 64, ... summed
// in that order, then a shuffle butterfly), once over the item table and once a call over the gathered user rows.  The recurrence over
// the C layers runs in the epilogue: about 6 C flops a pair; the item's scalars sit in LDS, the user's are uniform per wave.
//
// L = 1 has no layer past the split one (run_dcn.sh's own shape, 16-1-4-LN, is one): a VALU kernel, one pair a thread, as in the NCF files.
// NaN: a pair's values live on the two lanes of its item and in the scalars of its two rows: a NaN in an item's row reaches every score of
// that item and no other, a NaN in a user's row that user's row of scores only.  A user id outside the table is never dereferenced (Pu and
// the user scalars are indexed by the position in the batch): its row of scores is NaN.
#include <cmath>

#pragma clang fp contract(off)

#include "ncf_score_tile.h"

namespace pmgt {

static constexpr int DCS_RS = PMGT_DCN_SCORE_ROW_STRIDE;                    // floats per row of scalars: mu, q, d_0 .. d_C, zeros
static constexpr int DCS_MAX_CROSS = PMGT_DCN_MAX_CROSS, DCS_MAX_DEEP = PMGT_DCN_MAX_DEEP;
static_assert(DCS_RS % 4 == 0 && DCS_RS >= DCS_MAX_CROSS + 3, "the row of scalars holds mu, q and C + 1 dots");

struct DcsArgs {
    const float* w[DCS_MAX_DEEP];        // [i]: deep layer i's W [E >> i][E >> (i - 1)]; [0] is never read (the caller's split)
    const float* b[DCS_MAX_DEEP];
    const float* gamma[DCS_MAX_DEEP];    // LayerNorm of deep layer i over E >> i features
    const float* beta[DCS_MAX_DEEP];
    const float* wo_deep;                // output_layer.weight[D ..]: [2 F]
    const float* bo;                     // output_layer.bias
    const float* consts;                 // LayerNorm: K_c at [c], B_c at [PMGT_DCN_MAX_CROSS + c]
    const float* pu;                     // [n][E]
    const float* pi;                     // [I][E]
    const float* ur;                     // [n][DCS_RS]
    const float* ir;                     // [I][DCS_RS]
    const int64_t* users;                // [n]
    float* scores;                       // [n][row_stride]
    int64_t row_stride, user_num;
    float eps;
    int n, n_items, d, last, num_layers, cross, item_tiles;      // d = E, last = 2 F
};

struct DcsTile {
    const float* ur_s;      // LDS [TU][DCS_RS]
    const float* ir_s;      // LDS [32][DCS_RS]
    int r0, j0, wave, lane;
};

// z_cross of the pair whose user scalars are ur and item scalars ir (dcn_head.py's header)
template <bool LN> __device__ __forceinline__ float dcs_cross(const float* ur, const float* ir, const DcsArgs& a) {
    const int C = a.cross;
    if constexpr (LN) {
        const float mu_u = ur[0], mu_i = ir[0];
        const float m0 = (mu_u + mu_i) * 0.5f;
        const float du = mu_u - m0, di = mu_i - m0;
        const float v0 = ((ur[1] + ir[1]) + (float)a.d * (du * du + di * di)) * (1.f / (float)(2 * a.d));      // (powers of two)
        float s = ur[2] + ir[2];
        for (int c = 0; c < C; ++c) {
            const float k = s + 1.f;
            const float t = k / sqrtf((k * k) * v0 + a.eps);
            s = t * ((ur[3 + c] + ir[3 + c]) - m0 * a.consts[c]) + a.consts[DCS_MAX_CROSS + c];
        }
        return s;
    } else {
        float m = 1.f;
        for (int c = 0; c < C; ++c) m = m * (ur[2 + c] + ir[2 + c]) + 1.f;
        return m * (ur[2 + C] + ir[2 + C]);
    }
}

// the output layer on the last activations (features 32 b + rho(g) + 4 h of pair p in X[u][b][g]) plus the cross net; one store per pair
template <bool LN, int UW, int NB>
__device__ __forceinline__ void dcs_output_store(const f32x16 (&X)[UW][NB], const DcsArgs& a, const DcsTile& t) {
    const int p = t.lane & 31, h = t.lane >> 5, F2 = a.last;
    const float bo = a.bo[0];
    const float* ir = t.ir_s + p * DCS_RS;
#pragma unroll
    for (int u = 0; u < UW; ++u) {
        const int r = t.r0 + t.wave * UW + u;
        float s = 0.f;
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int f = b * 32 + rho(g) + 4 * h;
                if (f < F2) s = fmaf(a.wo_deep[f], X[u][b][g], s);
            }
        s += __shfl_xor(s, 32, 64);
        float z = (dcs_cross<LN>(t.ur_s + (t.wave * UW + u) * DCS_RS, ir, a) + s) + bo;
        if (r < a.n) {                               // (uniform per wave)
            const int64_t uid = a.users[r];
            if (uid < 0 || uid >= a.user_num) z = __builtin_nanf("");      // (the host surface refuses such ids)
        }
        const int j = t.j0 + p;
        if (h == 0 && r < a.n && j < a.n_items) a.scores[(int64_t)r * a.row_stride + j] = z;
    }
}

// L >= 2.  NB = 32-row blocks of layer 1's output (E / 2 rounded up to 32).  The file's own LDS tiles are the row scalars: item
// [32][DCS_RS] | user [TU][DCS_RS]; gamma0 / beta0 are reserved with and without LayerNorm
template <bool LN, int UW, int NB> __global__ __launch_bounds__(NCF_THREADS) void dcn_score_kernel(DcsArgs a) {
    extern __shared__ __align__(16) float smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = lane & 31, h = lane >> 5;
    const int d = a.d, TU = NCF_WAVES * UW;
    const TowerLds s = tower_lds(smem, d, TU, (NCF_ITEMS + TU) * DCS_RS, true);
    float* ir_s = s.own;                                     // [32][DCS_RS]
    float* ur_s = ir_s + NCF_ITEMS * DCS_RS;                 // [TU][DCS_RS]
    DcsTile t;
    t.j0 = (int)(blockIdx.x % (unsigned)a.item_tiles) * NCF_ITEMS;
    t.r0 = (int)(blockIdx.x / (unsigned)a.item_tiles) * TU;
    t.wave = wave;
    t.lane = lane;
    t.ur_s = ur_s;
    t.ir_s = ir_s;
    tower_load_tiles<LN, UW>(a, s, t.r0, t.j0, tid);
    for (int e = tid; e < NCF_ITEMS * DCS_RS; e += NCF_THREADS) {
        const int row = e / DCS_RS, c = e - row * DCS_RS, j = t.j0 + row;
        ir_s[e] = j < a.n_items ? a.ir[(int64_t)j * DCS_RS + c] : 0.f;
    }
    for (int e = tid; e < TU * DCS_RS; e += NCF_THREADS) {
        const int row = e / DCS_RS, c = e - row * DCS_RS, r = t.r0 + row;
        ur_s[e] = r < a.n ? a.ur[(int64_t)r * DCS_RS + c] : 0.f;
    }
    __syncthreads();                                         // the tiles are written
    const float* pu_w = s.pu_s + wave * UW * d;
    const float* pi_row = s.pi_s + p * (d + 1);
    float mean[UW], rstd[UW];
    if constexpr (LN) tower_row_stats<UW>(pu_w, pi_row, d, a.eps, h, mean, rstd);
    f32x16 acc[UW][NB];
    tower_first_layer<LN, UW, NB>(acc, a, s, pu_w, pi_row, mean, rstd, tid);
    tower_run_tail<LN, UW, NB>(acc, 2, a, s.ws, tid, [&](const auto& X) { dcs_output_store<LN>(X, a, t); });
}

// L = 1: z = wo_deep . relu([LN_0](Pu[r] + Pi[j])) + z_cross + bo over E = 2 F <= 128 features; one pair a thread, items on the lanes
template <bool LN> __global__ __launch_bounds__(NCF_THREADS) void dcn_score_l1_kernel(DcsArgs a) {
    const int64_t j = (int64_t)(blockIdx.x % (unsigned)a.item_tiles) * NCF_THREADS + threadIdx.x;
    const int r = (int)(blockIdx.x / (unsigned)a.item_tiles);
    if (j >= a.n_items || r >= a.n) return;
    const int E = a.d;
    const float* pu = a.pu + (int64_t)r * E;
    const float* pi = a.pi + j * E;
    float s = 0.f;
    if constexpr (LN) {
        const float* gamma = a.gamma[0];
        const float* beta = a.beta[0];
        const float inv = 1.f / (float)E;
        float m = 0.f, q = 0.f;
        for (int f = 0; f < E; ++f) m += pu[f] + pi[f];
        m *= inv;
        for (int f = 0; f < E; ++f) {
            const float c = (pu[f] + pi[f]) - m;
            q += c * c;
        }
        const float rstd = 1.f / sqrtf(q * inv + a.eps);
        for (int f = 0; f < E; ++f) s = fmaf(a.wo_deep[f], relu_keep_nan((((pu[f] + pi[f]) - m) * rstd) * gamma[f] + beta[f]), s);
    } else {
        for (int f = 0; f < E; ++f) s = fmaf(a.wo_deep[f], relu_keep_nan(pu[f] + pi[f]), s);
    }
    float z = (dcs_cross<LN>(a.ur + (int64_t)r * DCS_RS, a.ir + j * DCS_RS, a) + s) + a.bo[0];
    const int64_t uid = a.users[r];
    if (uid < 0 || uid >= a.user_num) z = __builtin_nanf("");
    a.scores[(int64_t)r * a.row_stride + j] = z;
}

struct DcsRowsArgs {
    const float* table;                  // [rows][E]
    const float* w[DCS_MAX_CROSS + 1];   // w_c + half E, c = 0 .. C (w_C = output_layer.weight[:D])
    const float* gamma[DCS_MAX_CROSS + 1];      // LayerNorm: [c] = gamma_(c-1) + half E for c >= 1
    float* out;                          // [rows][DCS_RS]
    int64_t rows;
    int E, cross, ln;
};

// one wave a row: lane holds the elements lane + 64 i, i < 4 (E <= 256); every sum runs over i in order, then the butterfly
__device__ __forceinline__ float dcs_wave_sum(float x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
__global__ __launch_bounds__(NCF_THREADS) void dcn_score_rows_kernel(DcsRowsArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * NCF_WAVES + (threadIdx.x >> 6);
    if (row >= a.rows) return;                               // (uniform per wave)
    const int E = a.E;
    float v[4];
    bool ok[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        ok[i] = lane + 64 * i < E;
        v[i] = ok[i] ? a.table[row * E + lane + 64 * i] : 0.f;
    }
    float res = 0.f;                                         // lane c of the wave ends with value c of the row
    if (a.ln) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) s += v[i];
        const float mu = dcs_wave_sum(s) * (1.f / (float)E);      // (E is a power of two)
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float c = ok[i] ? v[i] - mu : 0.f;
            q += c * c;
        }
        q = dcs_wave_sum(q);
        if (lane == 0) res = mu;
        if (lane == 1) res = q;
    }
    for (int c = 0; c <= a.cross; ++c) {
        const float* w = a.w[c];
        const float* ga = a.ln && c ? a.gamma[c] : nullptr;   // (uniform)
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (ok[i]) {
                const int k = lane + 64 * i;
                const float g = ga ? ga[k] * w[k] : w[k];
                s += v[i] * g;
            }
        s = dcs_wave_sum(s);
        if (lane == 2 + c) res = s;
    }
    if (lane < DCS_RS) a.out[row * DCS_RS + lane] = res;
}

// the covered shapes (check_dcn_covered) -> 0 or -2 in the name of `who`
static int dcs_shape(const pmgt_dcn_head* head, const char* who) {
    PMGT_CHECK(head != nullptr, -2, "%s: NULL head", who);
    const int F = head->factor_num, L = head->deep_layers, C = head->cross_layers, ln = head->use_layer_norm;
    PMGT_CHECK(F == 8 || F == 16 || F == 32 || F == 64, -2, "%s: factor_num = %d, covered: 8, 16, 32, 64", who, F);
    PMGT_CHECK(L >= 1 && L <= DCS_MAX_DEEP, -2, "%s: deep_layers = %d outside [1, %d]", who, L, DCS_MAX_DEEP);
    PMGT_CHECK((F << L) <= 256, -2, "%s: E = factor_num * 2^deep_layers = %d above 256", who, F << L);
    PMGT_CHECK(C >= 1 && C <= DCS_MAX_CROSS, -2, "%s: cross_layers = %d outside [1, %d]", who, C, DCS_MAX_CROSS);
    PMGT_CHECK(ln == 0 || ln == 1, -2, "%s: use_layer_norm = %d, expected 0 or 1", who, ln);
    PMGT_CHECK(head->user_num >= 1 && head->user_num <= 0x7FFFFFFELL && head->item_num >= 1 && head->item_num <= 0x7FFFFFFELL, -2,
               "%s: user_num = %lld or item_num = %lld outside [1, 2^31 - 2]", who, (long long)head->user_num, (long long)head->item_num);
    PMGT_CHECK(std::isfinite(head->layer_norm_eps) && head->layer_norm_eps >= 0.f, -2, "%s: layer_norm_eps = %g is not finite or negative", who,
               (double)head->layer_norm_eps);
    PMGT_CHECK(head->params && ((uintptr_t)head->params & 15) == 0, -2, "%s: the parameters must be non-NULL and 16-byte aligned", who);
    return 0;
}

template <bool LN, int UW, int NB> static int dcs_launch(const DcsArgs& a, hipStream_t st) {
    const int TU = NCF_WAVES * UW;
    const size_t smem = sizeof(float) * tower_lds_floats(a.d, TU, NB, (NCF_ITEMS + TU) * DCS_RS, true);
    // (the largest tile, E = 256, takes 61 952 bytes)
    return tower_launch<DcsArgs, dcn_score_kernel<LN, UW, NB>>("pmgt_dcn_score", a, TU, smem, 65536, st);
}

template <bool LN> static int dcs_dispatch(const DcsArgs& a, int L, int64_t n, int64_t n_items, hipStream_t st) {
    DcsArgs b = a;
    if (L == 1) {
        b.item_tiles = (int)((n_items + NCF_THREADS - 1) / NCF_THREADS);
        const int64_t grid = (int64_t)b.item_tiles * n;
        PMGT_CHECK(grid <= 0x7FFFFFFF, -2, "pmgt_dcn_score: %lld workgroups exceed the grid limit; split the users", (long long)grid);
        hipLaunchKernelGGL(dcn_score_l1_kernel<LN>, dim3((unsigned)grid), dim3(NCF_THREADS), 0, st, b);
        return 0;
    }
    b.item_tiles = (int)((n_items + NCF_ITEMS - 1) / NCF_ITEMS);
    // blocks of layer 1's output; users per wave: two at the widest layer (128 accumulator registers), four below
    if (b.d > 128) return dcs_launch<LN, 2, 4>(b, st);
    if (b.d > 64) return dcs_launch<LN, 4, 2>(b, st);
    return dcs_launch<LN, 4, 1>(b, st);
}

}  // namespace pmgt

using namespace pmgt;

extern "C" int pmgt_dcn_score_rows(const pmgt_dcn_head* head, const float* table, int64_t rows, int half, float* out, void* stream) {
    const char* who = "pmgt_dcn_score_rows";
    if (int rc = dcs_shape(head, who)) return rc;
    PMGT_CHECK(half == 0 || half == 1, -2, "%s: half = %d, expected 0 (users) or 1 (items)", who, half);
    PMGT_CHECK(rows >= 1 && rows <= 0x7FFFFFFELL, -2, "%s: %lld rows outside [1, 2^31 - 2]", who, (long long)rows);
    PMGT_CHECK(table && out && (((uintptr_t)table | (uintptr_t)out) & 15) == 0, -2, "%s: NULL or misaligned buffer", who);
    const int L = head->deep_layers, C = head->cross_layers, ln = head->use_layer_norm, E = head->factor_num << L;
    int64_t off[PMGT_DCN_TENSORS];
    PMGT_CHECK(pmgt_dcn_layout(head->factor_num, L, C, ln, head->user_num, head->item_num, off) > 0, -2, "%s: no layout for this shape", who);
    DcsRowsArgs a = {};
    a.table = table;
    for (int c = 0; c <= C; ++c) {
        a.w[c] = head->params + (c < C ? off[18 + 3 * c] : off[36]) + (int64_t)half * E;
        a.gamma[c] = ln && c ? head->params + off[19 + 3 * (c - 1)] + (int64_t)half * E : nullptr;
    }
    a.out = out;
    a.rows = rows;
    a.E = E, a.cross = C, a.ln = ln;
    const int64_t grid = (rows + NCF_WAVES - 1) / NCF_WAVES;
    hipLaunchKernelGGL(dcn_score_rows_kernel, dim3((unsigned)grid), dim3(NCF_THREADS), 0, (hipStream_t)stream, a);
    PMGT_LAUNCH_OK();
    return 0;
}

extern "C" int pmgt_dcn_score(const pmgt_dcn_head* head, const float* pu, const float* pi, const float* user_rows, const float* item_rows,
                              const float* consts, const int64_t* users, int64_t n, int64_t n_items, float* scores, int64_t row_stride,
                              void* stream) {
    const char* who = "pmgt_dcn_score";
    if (int rc = dcs_shape(head, who)) return rc;
    const int F = head->factor_num, L = head->deep_layers, C = head->cross_layers, ln = head->use_layer_norm, E = F << L;
    PMGT_CHECK(n >= 1 && n <= PMGT_NCF_MAX_USERS, -2, "%s: n = %lld users outside [1, %d]", who, (long long)n, PMGT_NCF_MAX_USERS);
    PMGT_CHECK(n_items >= 1 && n_items <= 0x7FFFFFFELL, -2, "%s: %lld items outside [1, 2^31 - 2]", who, (long long)n_items);
    PMGT_CHECK(row_stride >= n_items, -2, "%s: row_stride = %lld below the %lld items", who, (long long)row_stride, (long long)n_items);
    PMGT_CHECK(pu && pi && user_rows && item_rows && users && scores && (!ln || consts), -2, "%s: NULL buffer", who);
    PMGT_CHECK((((uintptr_t)pu | (uintptr_t)pi | (uintptr_t)user_rows | (uintptr_t)item_rows) & 15) == 0 &&
                   (((uintptr_t)scores | (uintptr_t)consts) & 3) == 0 && ((uintptr_t)users & 7) == 0,
               -2, "%s: misaligned buffer (pu, pi and the row scalars: 16 bytes; users: 8; scores and consts: 4)", who);
    int64_t off[PMGT_DCN_TENSORS];
    PMGT_CHECK(pmgt_dcn_layout(F, L, C, ln, head->user_num, head->item_num, off) > 0, -2, "%s: no layout for this shape", who);
    const float* P = head->params;
    DcsArgs a = {};
    for (int l = 0; l < L; ++l) {
        a.w[l] = P + off[2 + 4 * l], a.b[l] = P + off[3 + 4 * l];
        if (ln) a.gamma[l] = P + off[4 + 4 * l], a.beta[l] = P + off[5 + 4 * l];
    }
    a.wo_deep = P + off[36] + 2 * E;
    a.bo = P + off[37];
    a.consts = consts;
    a.pu = pu, a.pi = pi, a.ur = user_rows, a.ir = item_rows;
    a.users = users;
    a.scores = scores;
    a.row_stride = row_stride;
    a.user_num = head->user_num;
    a.eps = head->layer_norm_eps;
    a.n = (int)n, a.n_items = (int)n_items;
    a.d = E, a.last = 2 * F, a.num_layers = L, a.cross = C;
    const int rc = ln ? dcs_dispatch<true>(a, L, n, n_items, (hipStream_t)stream) : dcs_dispatch<false>(a, L, n, n_items, (hipStream_t)stream);
    if (rc) return rc;
    PMGT_LAUNCH_OK();
    return 0;
}
