// Item-by-item scoring from one embedding table (pmgt_item_sim_norms, pmgt_item_sim_score of include/pmgt_capi.h): the score of every
// (query item, catalogue item) pair as the dot product or the cosine of their rows -- the quantity the graph-structure objective trains
// (pmgt/pmgt/losses.py PMGTGraphConstructLoss: F.normalize, then a dot product).  Kept out of csrc/ for ncf_score.hip's reason: the measured
// step launches nothing of this.
//
// THE SCORE.  dot(i, j) = the fp32 fmaf chain over k = 0 .. d - 1 in ascending order from 0, on the exact f32-input MFMA
// (v_mfma_f32_32x32x2_f32: bitwise that chain).  metric "dot": s = dot.  metric "cosine": s = (dot * inv[min(i, j)]) * inv[max(i, j)],
// each product rounded to fp32, inv[j] = 1 / max(|x_j|, eps) from pmgt_item_sim_norms.  A product commutes and the scalings are applied in
// the order of the two ITEM IDS, not of (query, candidate), so s(i, j) and s(j, i) have the same bits; an output element reads row i and
// row j of the table and nothing else, in an order that does not depend on the tile it falls into, so the bits do not depend on n, on the
// order of the queries or on how the catalogue is cut into calls, and a NaN in row j reaches the scores of row j and column j only.
// Past d both operands are zero: fmaf(0, 0, acc) leaves acc (at most it turns a -0 that an underflow left into +0, which no order sees).
//
// TILE (ncf_score_tile.h's pattern, read against the LDS and MFMA sections of the kernel guides).  A workgroup of 4 waves owns TM queries x TN
// candidates; k-chunks of 32 columns of BOTH operands go through LDS as [row][33] floats (the odd stride makes the column read of a
// k-step conflict-free but for one bank pair); the next chunk's global loads are issued before the MFMAs of the current one and stored
// after them (16-byte loads where d is a multiple of 4 and the table is aligned, single floats else: the same values in the same places).  The query rows are gathered through `queries` straight from the table, the candidates come from the same table: no
// gathered and no normalised copy exists.  Two shapes, chosen by n alone (the bits are the same):
//   n > 32:   128 x 128, waves 2 x 2, each wave 2 x 2 blocks of 32 x 32 (64 accumulator registers): every operand read from LDS feeds two
//             MFMAs, 4 independent accumulators a wave keep the 64-cycle MFMA issue back to back; 137 VGPRs and 34 KiB of LDS leave 3 workgroups a CU
//   n <= 32:  32 x 256, waves 1 x 4, each wave 1 x 2 blocks: a single query or a short list does not pay for 128 query rows
// In a 32 x 32 result block the CANDIDATE is on the lane (j = lane & 31) and the query row in the register (row rho(g) + 4 (lane >> 5)),
// so one store instruction writes two runs of 32 consecutive floats.  The epilogue is the two scalings and the store; output offsets are
// 64-bit.  Rows past n and candidates past n_items are zeros: computed, never stored.  A query id outside [0, n_items) is never
// dereferenced: its operand row is zeros and its row of scores NaN (the rule predict_store keeps for a bad user).  No atomics anywhere.
//
// NORMS.  sum_k x[k]^2 is THE DOT PRODUCT'S OWN CHAIN, fmaf over k ascending from 0, so it has the bits of dot(j, j): the rounding of the
// long sum cancels between a dot product and the norms wherever two rows are alike, and s(j, j) is 1 to a few roundings (with a tree for
// the norms s(j, j) carries the whole error of the sequential sum: 2^-20 at d = 1024 on a standard normal table).  A chain is one
// thread's work: 64 rows a wave at every d, a workgroup of 256 rows; the k-chunks go through LDS so that the global reads stay coalesced.
#include "ncf_head.h"

namespace pmgt {

static constexpr int SIM_THREADS = 256, SIM_CHUNK = 32, SIM_STRIDE = SIM_CHUNK + 1, SIM_MAX_D = PMGT_ITEM_SIM_MAX_D;

struct SimArgs {
    const float* table;        // [n_items][d]
    const float* inv;          // [n_items] or NULL (metric "dot")
    const int64_t* queries;    // [n]
    float* scores;             // [n][row_stride]
    int64_t row_stride;
    int n, n_items, d, item_tiles;
};

__global__ __launch_bounds__(SIM_THREADS) void item_sim_norms_kernel(const float* __restrict__ table, int n_items, int d, float eps,
                                                                     float* __restrict__ inv) {
    __shared__ float ws[SIM_THREADS * SIM_STRIDE];           // 256 rows x one k-chunk
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * SIM_THREADS;
    float s = 0.f;
    for (int k0 = 0; k0 < d; k0 += SIM_CHUNK) {
        __syncthreads();                                     // every thread is done with the previous chunk
#pragma unroll 8
        for (int i = 0; i < SIM_CHUNK; ++i) {                // coalesced: 32 consecutive floats of a row per 32 threads
            const int e = tid + SIM_THREADS * i, c = e & 31, m = e >> 5;
            ws[m * SIM_STRIDE + c] = (row0 + m < n_items && k0 + c < d) ? table[(row0 + m) * d + k0 + c] : 0.f;
        }
        __syncthreads();
        const int kc = min(SIM_CHUNK, d - k0);
        for (int c = 0; c < kc; ++c) {                       // thread t walks row t in ascending k (odd stride: no bank conflict)
            const float x = ws[tid * SIM_STRIDE + c];
            s = fmaf(x, x, s);
        }
    }
    if (row0 + tid < n_items) {
        const float nrm = sqrtf(s);
        inv[row0 + tid] = 1.f / (nrm < eps ? eps : nrm);     // (a NaN norm stays a NaN)
    }
}

// rows [row0, row0 + ROWS) x k-columns [k0, k0 + 32) of the operand, zero past the live rows and past d: global -> registers
// ids == NULL: the rows are the table's own (candidates); else they are gathered through the LDS copy of the tile's query ids (< 0: none)
// VEC (d a multiple of 4, the table 16-byte aligned): one 16-byte load per 4 columns, 8 threads a row; else one float a thread, 32 a row
template <int ROWS, bool VEC> __device__ __forceinline__ void sim_fetch(float (&st)[ROWS / 8], const float* __restrict__ table, const int* ids,
                                                                         int64_t row0, int live, int d, int k0, int tid) {
    if constexpr (VEC) {
#pragma unroll
        for (int i = 0; i < ROWS / 32; ++i) {
            const int e = tid + SIM_THREADS * i, c = (e & 7) * 4, m = e >> 3;
            int64_t row = -1;
            if (ids) row = ids[m];
            else if (row0 + m < live) row = row0 + m;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row >= 0 && k0 + c < d) v = *reinterpret_cast<const float4*>(table + row * d + k0 + c);
            st[4 * i] = v.x, st[4 * i + 1] = v.y, st[4 * i + 2] = v.z, st[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < ROWS / 8; ++i) {
            const int e = tid + SIM_THREADS * i, c = e & 31, m = e >> 5;
            int64_t row = -1;
            if (ids) row = ids[m];
            else if (row0 + m < live) row = row0 + m;
            st[i] = (row >= 0 && k0 + c < d) ? table[row * d + k0 + c] : 0.f;
        }
    }
}
template <int ROWS, bool VEC> __device__ __forceinline__ void sim_store(const float (&st)[ROWS / 8], float* ws, int tid) {
    if constexpr (VEC) {
#pragma unroll
        for (int i = 0; i < ROWS / 32; ++i) {
            const int e = tid + SIM_THREADS * i, c = (e & 7) * 4, m = e >> 3;
#pragma unroll
            for (int t = 0; t < 4; ++t) ws[m * SIM_STRIDE + c + t] = st[4 * i + t];
        }
    } else {
#pragma unroll
        for (int i = 0; i < ROWS / 8; ++i) {
            const int e = tid + SIM_THREADS * i, c = e & 31, m = e >> 5;
            ws[m * SIM_STRIDE + c] = st[i];
        }
    }
}

// waves WM x WN (= 4), blocks of 32 x 32 per wave BM x BN: the tile is TM = 32 WM BM queries x TN = 32 WN BN candidates
template <int WM, int WN, int BM, int BN, bool VEC> __global__ __launch_bounds__(SIM_THREADS) void item_sim_score_kernel(SimArgs a) {
    constexpr int TM = 32 * WM * BM, TN = 32 * WN * BN;
    __shared__ float qs[TM * SIM_STRIDE];
    __shared__ float cs[TN * SIM_STRIDE];
    __shared__ int qid[TM];                                  // the tile's query ids; -1 = past n, -2 = an id outside the table (its row is NaN)
    __shared__ float qinv[TM];                               // their inverse norms (cosine)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = lane & 31, h = lane >> 5;
    const int wm = wave / WN, wn = wave % WN;
    const int64_t j0 = (int64_t)(blockIdx.x % (unsigned)a.item_tiles) * TN;
    const int r0 = (int)(blockIdx.x / (unsigned)a.item_tiles) * TM;
    const int d = a.d;
    for (int m = tid; m < TM; m += SIM_THREADS) {
        int id = -1;
        if (r0 + m < a.n) {
            const int64_t q = a.queries[r0 + m];
            id = (q >= 0 && q < a.n_items) ? (int)q : -2;
        }
        qid[m] = id;
        qinv[m] = (id >= 0 && a.inv) ? a.inv[id] : 0.f;
    }
    __syncthreads();
    f32x16 acc[BM][BN];
#pragma unroll
    for (int bm = 0; bm < BM; ++bm)
#pragma unroll
        for (int bn = 0; bn < BN; ++bn)
#pragma unroll
            for (int g = 0; g < 16; ++g) acc[bm][bn][g] = 0.f;
    float sq[TM / 8], sc[TN / 8];
    sim_fetch<TM, VEC>(sq, a.table, qid, 0, 0, d, 0, tid);
    sim_fetch<TN, VEC>(sc, a.table, nullptr, j0, a.n_items, d, 0, tid);
    const float* qw = qs + (wm * BM * 32 + p) * SIM_STRIDE + h;
    const float* cw = cs + (wn * BN * 32 + p) * SIM_STRIDE + h;
    for (int k0 = 0; k0 < d; k0 += SIM_CHUNK) {
        __syncthreads();                                     // every wave is done with the previous chunk
        sim_store<TM, VEC>(sq, qs, tid);
        sim_store<TN, VEC>(sc, cs, tid);
        __syncthreads();
        if (k0 + SIM_CHUNK < d) {
            sim_fetch<TM, VEC>(sq, a.table, qid, 0, 0, d, k0 + SIM_CHUNK, tid);
            sim_fetch<TN, VEC>(sc, a.table, nullptr, j0, a.n_items, d, k0 + SIM_CHUNK, tid);
        }
        const int kc = min(SIM_CHUNK, d - k0);
        for (int s0 = 0; s0 < kc; s0 += 8)                   // (uniform; the k-steps past d multiply zeros)
#pragma unroll
            for (int s = s0; s < s0 + 8; s += 2) {
                float qa[BM], cb[BN];
#pragma unroll
                for (int bm = 0; bm < BM; ++bm) qa[bm] = qw[bm * 32 * SIM_STRIDE + s];
#pragma unroll
                for (int bn = 0; bn < BN; ++bn) cb[bn] = cw[bn * 32 * SIM_STRIDE + s];
#pragma unroll
                for (int bm = 0; bm < BM; ++bm)
#pragma unroll
                    for (int bn = 0; bn < BN; ++bn) acc[bm][bn] = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[bm], cb[bn], acc[bm][bn], 0, 0, 0);
            }
    }
    // epilogue: register g of block (bm, bn) = query row 32 (wm BM + bm) + rho(g) + 4 h, candidate j0 + 32 (wn BN + bn) + p
    const bool cosine = a.inv != nullptr;
#pragma unroll
    for (int bn = 0; bn < BN; ++bn) {
        const int64_t j = j0 + (wn * BN + bn) * 32 + p;
        if (j >= a.n_items) continue;
        const float inv_j = cosine ? a.inv[j] : 1.f;
#pragma unroll
        for (int bm = 0; bm < BM; ++bm)
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int m = (wm * BM + bm) * 32 + rho(g) + 4 * h, r = r0 + m;
                if (r >= a.n) continue;
                const int i = qid[m];
                float s = acc[bm][bn][g];
                if (i < 0) {
                    s = __builtin_nanf("");
                } else if (cosine) {
                    const float inv_i = qinv[m];
                    s = i <= j ? (s * inv_i) * inv_j : (s * inv_j) * inv_i;
                }
                a.scores[(int64_t)r * a.row_stride + j] = s;
            }
    }
}

template <int WM, int WN, int BM, int BN, bool VEC> static int sim_launch(SimArgs& a, hipStream_t st) {
    constexpr int TM = 32 * WM * BM, TN = 32 * WN * BN;
    static_assert(WM * WN * 64 == SIM_THREADS, "four waves");
    a.item_tiles = (int)(((int64_t)a.n_items + TN - 1) / TN);
    const int64_t grid = (int64_t)a.item_tiles * ((a.n + TM - 1) / TM);
    PMGT_CHECK(grid <= 0x7FFFFFFF, -2, "pmgt_item_sim_score: %lld workgroups exceed the grid limit; split the queries", (long long)grid);
    hipLaunchKernelGGL((item_sim_score_kernel<WM, WN, BM, BN, VEC>), dim3((unsigned)grid), dim3(SIM_THREADS), 0, st, a);
    return 0;
}

}  // namespace pmgt

using namespace pmgt;

extern "C" int pmgt_item_sim_norms(const float* table, int64_t n_items, int d, float eps, float* inv_norm, void* stream) {
    PMGT_CHECK(d >= 1 && d <= SIM_MAX_D, -2, "pmgt_item_sim_norms: d = %d outside [1, %d]", d, SIM_MAX_D);
    PMGT_CHECK(n_items >= 1 && n_items <= 0x7FFFFFFELL, -2, "pmgt_item_sim_norms: %lld items outside [1, 2^31 - 2]", (long long)n_items);
    PMGT_CHECK(eps > 0.f && eps <= 3.0e38f, -2, "pmgt_item_sim_norms: eps = %g is not a positive finite number", (double)eps);
    PMGT_CHECK(table && inv_norm, -2, "pmgt_item_sim_norms: NULL buffer");
    PMGT_CHECK((((uintptr_t)table | (uintptr_t)inv_norm) & 3) == 0, -2, "pmgt_item_sim_norms: misaligned buffer");
    const int64_t grid = (n_items + SIM_THREADS - 1) / SIM_THREADS;
    hipLaunchKernelGGL(item_sim_norms_kernel, dim3((unsigned)grid), dim3(SIM_THREADS), 0, (hipStream_t)stream, table, (int)n_items, d, eps, inv_norm);
    PMGT_LAUNCH_OK();
    return 0;
}

extern "C" int pmgt_item_sim_score(const float* table, const float* inv_norm, const int64_t* queries, int64_t n, int64_t n_items, int d,
                                   float* scores, int64_t row_stride, void* stream) {
    PMGT_CHECK(d >= 1 && d <= SIM_MAX_D, -2, "pmgt_item_sim_score: d = %d outside [1, %d]", d, SIM_MAX_D);
    PMGT_CHECK(n >= 1 && n <= PMGT_NCF_MAX_USERS, -2, "pmgt_item_sim_score: n = %lld queries outside [1, %d]", (long long)n, PMGT_NCF_MAX_USERS);
    PMGT_CHECK(n_items >= 1 && n_items <= 0x7FFFFFFELL, -2, "pmgt_item_sim_score: %lld items outside [1, 2^31 - 2]", (long long)n_items);
    PMGT_CHECK(row_stride >= n_items, -2, "pmgt_item_sim_score: row_stride = %lld below the %lld items", (long long)row_stride, (long long)n_items);
    PMGT_CHECK(table && queries && scores, -2, "pmgt_item_sim_score: NULL buffer");
    PMGT_CHECK((((uintptr_t)table | (uintptr_t)inv_norm | (uintptr_t)scores) & 3) == 0 && ((uintptr_t)queries & 7) == 0, -2,
               "pmgt_item_sim_score: misaligned buffer");
    SimArgs a;
    a.table = table;
    a.inv = inv_norm;
    a.queries = queries;
    a.scores = scores;
    a.row_stride = row_stride;
    a.n = (int)n;
    a.n_items = (int)n_items;
    a.d = d;
    a.item_tiles = 0;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (d & 3) == 0 && ((uintptr_t)table & 15) == 0;      // every row then starts on 16 bytes
    int rc;
    if (n > 32) rc = vec ? sim_launch<2, 2, 2, 2, true>(a, st) : sim_launch<2, 2, 2, 2, false>(a, st);
    else rc = vec ? sim_launch<1, 4, 1, 2, true>(a, st) : sim_launch<1, 4, 1, 2, false>(a, st);
    if (rc) return rc;
    PMGT_LAUNCH_OK();
    return 0;
}
