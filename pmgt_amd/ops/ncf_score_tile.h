// What the two scoring files share (ncf_score.hip: the head of PMGT_NCF; ncf_model_score.hip: the stand-alone NCF class with LayerNorm): the
// shape of the tile, the weight chunks streamed through LDS, the bias as the accumulators' initial value, and the predict layer with the GMF
// branch.  ncf_score.hip's header states the design.  Every function is inlined into its caller; Args is the caller's argument struct (wp,
// bp, gu, users, scores, row_stride, user_num, n, n_items, factor are read).
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

}  // namespace pmgt
