// Top-N ranking metrics on the device (pmgt_rank_* of include/pmgt_capi.h): nDCG@k, Recall@k and the per-user loss of the reference's
// ranking evaluation (`NCFTrainerModel._validation_and_test_step` / `validation_epoch_end`, pmgt/ncf/trainer.py:202-254, over `get_ndcg` /
// `get_recall`, pmgt/metrics.py:16-37) without its Python iteration, topk, .item() and device-to-host copy per user.
// Kept out of csrc/ for eval_metrics.hip's reason: the measured step launches nothing of this.
//
// THE TIE RULE.  With key = eval_key() of eval_metrics.h (order-preserving image of the fp32 score, -0.0 folded onto +0.0, +-inf at the ends),
// the rank of candidate p of a row is
//       rank(p) = #{c : key(c) > key(p)} + #{c < p : key(c) == key(p)}
// so the ranks of a row form a permutation and, among equal scores, the LOWER CANDIDATE INDEX ranks first.  torch.topk leaves the order of
// ties unspecified; this is the project's rule, and the host path (pmgt_amd.evaluation.ranking_metrics_host) states the same one.
//
// append: one 256-thread workgroup per user row.  The row's keys, the list of its positives and the discount table sit in LDS; the positives
//   (compacted by ballot and popcount, one LDS atomic per wave and round) are dealt out to the four waves, a wave counts one positive's
//   rank with lane-strided compares and a wave reduction (no sort: only positives need ranks), and a hit below max(ks) sets its byte in a rank-indexed array.  Wave 0 then walks that array in ascending rank and
//   adds disc[rank] in fp64, emitting dcg and the hit count at each cut-off: one walk serves all k, and the adds come in the reference's order.
//   The device evaluates no logarithm: disc[r] = 1 / log2(r + 2) and idcg = cumsum(disc) are the host's tables, uploaded by reset; with the
//   ascending adds and ONE IEEE division per metric the per-user values are the reference's bit for bit.
//   The per-user loss is the mean of max(x, 0) - x y + log1pf(expf(-|x|)), y = (label != 0), over the live candidates in fp32: thread
//   partials in candidate order, a fixed shuffle tree, the four wave sums in order.
// reduce: one workgroup per quantity; thread t adds the users t, t + 256, ... in ascending order, then a fixed tree over the 256 partials.
//   No floating-point atomic anywhere: results are bitwise repeatable and do not depend on how the users were split over appends.
#include <algorithm>

#include "ranking_metrics.h"

namespace pmgt {

struct RankKs {
    int n_k;
    int ks[RANK_MAX_KS];
};
struct RankTableChunk {
    double disc[RANK_TABLE_CHUNK];
    double idcg[RANK_TABLE_CHUNK];
};

__device__ __forceinline__ bool rank_config_ok(const RankConfig& c, int64_t max_users) {
    if (c.magic != RANK_MAGIC || c.max_users != max_users || c.n_k < 1 || c.n_k > RANK_MAX_KS) return false;
    int prev = 0;
    for (int i = 0; i < c.n_k; ++i) {
        if (c.ks[i] <= prev || c.ks[i] > RANK_MAX_K) return false;
        prev = c.ks[i];
    }
    return c.max_k == prev;
}

// ---- reset -----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void rank_reset_kernel(void* ws, int64_t max_users, RankKs ks) {
    const RankWorkspace w = rank_carve(ws, max_users, ks.n_k);
    const int t = threadIdx.x;
    if (t < (int)(RANK_HEADER_BYTES / 8)) w.u[t] = 0ull;
    if (t == 0) {
        RankConfig c;
        c.max_users = max_users;
        c.magic = RANK_MAGIC;
        c.n_k = ks.n_k;
        c.max_k = ks.ks[ks.n_k - 1];
        for (int i = 0; i < RANK_MAX_KS; ++i) c.ks[i] = i < ks.n_k ? ks.ks[i] : 0;
        c.reserved[0] = c.reserved[1] = c.reserved[2] = 0;
        *w.cfg = c;
    }
}

// entries [first, first + n) of both tables, carried in the kernel arguments: stream-ordered like any launch, no host buffer outlives the call
__global__ __launch_bounds__(RANK_TABLE_CHUNK) void rank_table_kernel(double* __restrict__ disc, double* __restrict__ idcg, int first, int n,
                                                                      RankTableChunk chunk) {
    const int t = threadIdx.x;
    if (t < n && first + t < RANK_MAX_K) {
        disc[first + t] = chunk.disc[t];
        idcg[first + t] = chunk.idcg[t];
    }
}

// ---- append: one workgroup per user row ------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__global__ __launch_bounds__(RANK_THREADS) void rank_append_kernel(void* ws, int64_t max_users, const float* __restrict__ logits,
                                                                   const float* __restrict__ labels, const int32_t* __restrict__ counts,
                                                                   int row_stride, int64_t user_offset, int n_users) {
#pragma clang fp contract(off)      // the loss term is rounded operation by operation: the formula as written
    __shared__ uint32_t keys[RANK_MAX_ROW];          // 16 KiB
    __shared__ double disc_s[RANK_MAX_K];            // 8 KiB
    __shared__ uint16_t plist[RANK_MAX_ROW];         // 8 KiB: candidate indices of the positives, in no particular order
    __shared__ uint8_t hit[RANK_MAX_K];              // hit[r] = a positive has rank r
    __shared__ float wloss[RANK_WAVES];
    __shared__ int npos_s, nan_s;
    __shared__ RankConfig cfg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x;
    if (row >= n_users) return;                      // (uniform)
    if (tid == 0) {
        cfg = *(const RankConfig*)((const char*)ws + RANK_HEADER_BYTES);
        npos_s = 0;
        nan_s = 0;
    }
    __syncthreads();
    if (!rank_config_ok(cfg, max_users)) return;     // (uniform) no reset on this workspace: nothing is written
    const int64_t slot = user_offset + row;
    if (slot < 0 || slot >= max_users) return;       // (the host refuses this; never write outside the records)
    const RankWorkspace w = rank_carve(ws, max_users, cfg.n_k);
    const int max_k = cfg.max_k;
    int count = counts ? counts[row] : row_stride;
    count = min(max(count, 0), min(row_stride, RANK_MAX_ROW));      // entries past the count are padding: never read
    for (int r = tid; r < max_k; r += RANK_THREADS) {
        disc_s[r] = w.disc[r];
        hit[r] = 0;
    }
    const float* x_row = logits + (int64_t)row * row_stride;
    const float* y_row = labels + (int64_t)row * row_stride;
    float part = 0.f;
    bool bad = false;
    const unsigned long long lanes_below = (1ull << lane) - 1ull;
    for (int c0 = 0; c0 < count; c0 += RANK_THREADS) {       // (uniform trip count: the ballot below sees whole waves)
        const int c = c0 + tid;
        const bool valid = c < count;
        const float x = valid ? x_row[c] : 0.f;
        const float y = (valid && y_row[c] != 0.f) ? 1.f : 0.f;      // positive iff label != 0; the loss sees 0 or 1 whatever the value
        // the wave's positives take consecutive places of the list: one LDS atomic per wave and round, not one per positive
        const unsigned long long pm = __builtin_amdgcn_ballot_w64(y != 0.f);
        int base = 0;
        if (lane == 0 && pm) base = atomicAdd(&npos_s, (int)__popcll(pm));
        base = __shfl(base, 0, 64);
        if (y != 0.f) plist[base + (int)__popcll(pm & lanes_below)] = (uint16_t)c;
        if (valid) {
            const bool isnan_x = x != x;
            bad |= isnan_x;
            keys[c] = isnan_x ? 0xFFFFFFFFu : eval_key(x);     // not a key of any score: eval_key() of +Inf is 0xFF800000
            const float term = (fmaxf(x, 0.f) - x * y) + log1pf(expf(-fabsf(x)));
            part = part + term;
        }
    }
    if (bad) nan_s = 1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part = part + __shfl_xor(part, o, 64);
    if (lane == 0) wloss[wave] = part;
    __syncthreads();
    const int n_pos = npos_s;                        // <= count <= RANK_MAX_ROW
    for (int j = wave; j < n_pos; j += RANK_WAVES) {
        const int p = plist[j];
        const uint32_t kp = keys[p];
        int above = 0;
        for (int c = lane; c < count; c += 64) {
            const uint32_t k = keys[c];
            above += (k > kp || (k == kp && c < p)) ? 1 : 0;
        }
        above = wave_sum_i32(above);
        if (lane == 0 && above < max_k) hit[above] = 1;
    }
    __syncthreads();
    if (wave != 0) return;
    // wave 0, every lane the same values: the hit ranks in ascending order, dcg and hits emitted where a cut-off is passed
    double dcg = 0.0;
    int hits = 0, ki = 0;
    const int n_k = cfg.n_k;
    for (int base = 0; base < max_k; base += 64) {
        const int r = base + lane;
        unsigned long long m = __builtin_amdgcn_ballot_w64(r < max_k && hit[r] != 0);
        while (ki < n_k && cfg.ks[ki] <= base + 64) {
            const int kb = cfg.ks[ki] - base;        // 1 .. 64: ranks base .. base + kb - 1 are below this cut-off
            const unsigned long long below = kb >= 64 ? ~0ull : ((1ull << kb) - 1ull);
            unsigned long long take = m & below;
            m &= ~below;
            while (take) {
                dcg = dcg + disc_s[base + __builtin_ctzll(take)];
                ++hits;
                take &= take - 1ull;
            }
            if (lane == 0) {
                const int64_t at = (int64_t)ki * w.capr + slot;
                if (n_pos > 0) {
                    w.recall[at] = (double)hits / (double)n_pos;
                    w.ndcg[at] = dcg / w.idcg[min(n_pos, cfg.ks[ki]) - 1];
                } else {
                    w.recall[at] = 0.0;
                    w.ndcg[at] = 0.0;
                }
            }
            ++ki;
        }
        while (m) {
            dcg = dcg + disc_s[base + __builtin_ctzll(m)];
            ++hits;
            m &= m - 1ull;
        }
    }
    if (lane == 0) {
        const float total = ((wloss[0] + wloss[1]) + wloss[2]) + wloss[3];
        w.loss[slot] = count > 0 ? total / (float)count : 0.f;
        w.n_pos[slot] = n_pos;
        w.flags[slot] = (nan_s ? RANK_FLAG_NAN : 0u) | (n_pos == 0 ? RANK_FLAG_EMPTY : 0u);      // (clears RANK_FLAG_UNWRITTEN)
    }
}

// ---- reduce: workgroup q sums one quantity over the users 0 .. n in a fixed order ------------------------------------------------------------
__global__ __launch_bounds__(RANK_THREADS) void rank_reduce_kernel(void* ws, int64_t max_users, int64_t n) {
    __shared__ double wsum[RANK_WAVES];
    __shared__ unsigned long long wcnt[RANK_WAVES][3];
    __shared__ RankConfig cfg;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.x;
    if (tid == 0) cfg = *(const RankConfig*)((const char*)ws + RANK_HEADER_BYTES);
    __syncthreads();
    if (!rank_config_ok(cfg, max_users) || n < 1 || n > max_users) return;
    const int n_k = cfg.n_k;
    if (q > 2 * n_k + 1) return;
    const RankWorkspace w = rank_carve(ws, max_users, n_k);
    if (q == 2 * n_k + 1) {             // the integers
        unsigned long long n_nan = 0, n_empty = 0, n_unwritten = 0;
        for (int64_t u = tid; u < n; u += RANK_THREADS) {
            const uint32_t f = w.flags[u];
            n_nan += (f & RANK_FLAG_NAN) ? 1ull : 0ull;
            n_empty += (f & RANK_FLAG_EMPTY) ? 1ull : 0ull;
            n_unwritten += (f & RANK_FLAG_UNWRITTEN) ? 1ull : 0ull;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            n_nan += __shfl_xor(n_nan, o, 64);
            n_empty += __shfl_xor(n_empty, o, 64);
            n_unwritten += __shfl_xor(n_unwritten, o, 64);
        }
        if (lane == 0) { wcnt[wave][0] = n_nan; wcnt[wave][1] = n_empty; wcnt[wave][2] = n_unwritten; }
        __syncthreads();
        if (tid == 0) {
            w.u[9] = (unsigned long long)n;
            w.u[10] = wcnt[0][0] + wcnt[1][0] + wcnt[2][0] + wcnt[3][0];
            w.u[11] = wcnt[0][1] + wcnt[1][1] + wcnt[2][1] + wcnt[3][1];
            w.u[12] = wcnt[0][2] + wcnt[1][2] + wcnt[2][2] + wcnt[3][2];
        }
        return;
    }
    const double* src = q < n_k ? w.ndcg + (int64_t)q * w.capr : (q < 2 * n_k ? w.recall + (int64_t)(q - n_k) * w.capr : nullptr);
    double s = 0.0;
    for (int64_t u = tid; u < n; u += RANK_THREADS) s = s + (src ? src[u] : (double)w.loss[u]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    if (tid == 0) {
        const double total = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
        w.sums[q < n_k ? q : (q < 2 * n_k ? RANK_MAX_KS + (q - n_k) : 2 * RANK_MAX_KS)] = total;
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------------
static int rank_check(const void* ws, int64_t max_users, const char* who) {
    PMGT_CHECK(ws != nullptr, -2, "%s: NULL workspace", who);
    PMGT_CHECK(max_users >= 1 && max_users <= RANK_MAX_USERS, -2, "%s: max_users = %lld outside [1, %lld]", who, (long long)max_users,
               (long long)RANK_MAX_USERS);
    PMGT_CHECK(((uintptr_t)ws & 15) == 0, -2, "%s: the workspace must be 16-byte aligned", who);
    return 0;
}

static int rank_check_ks(const int* ks, int n_k, const char* who) {
    PMGT_CHECK(n_k >= 1 && n_k <= RANK_MAX_KS, -2, "%s: n_k = %d outside [1, %d]", who, n_k, RANK_MAX_KS);
    PMGT_CHECK(ks != nullptr, -2, "%s: NULL ks", who);
    int prev = 0;
    for (int i = 0; i < n_k; ++i) {
        PMGT_CHECK(ks[i] > prev && ks[i] <= RANK_MAX_K, -2, "%s: ks[%d] = %d: the cut-offs must be strictly increasing in [1, %d]", who, i, ks[i],
                   RANK_MAX_K);
        prev = ks[i];
    }
    return 0;
}

}  // namespace pmgt

using namespace pmgt;

extern "C" {

int64_t pmgt_rank_workspace_bytes(int64_t max_users, int n_k) {
    if (max_users < 1 || max_users > RANK_MAX_USERS || n_k < 1 || n_k > RANK_MAX_KS) return -2;
    return rank_carve(nullptr, max_users, n_k).bytes;
}

int pmgt_rank_reset(void* ws, int64_t max_users, const int* ks, int n_k, const double* disc, const double* idcg, void* stream) {
    if (int rc = rank_check(ws, max_users, "pmgt_rank_reset")) return rc;
    if (int rc = rank_check_ks(ks, n_k, "pmgt_rank_reset")) return rc;
    PMGT_CHECK(disc && idcg, -2, "pmgt_rank_reset: NULL table");
    PMGT_CHECK(((uintptr_t)disc & 7) == 0 && ((uintptr_t)idcg & 7) == 0, -2, "pmgt_rank_reset: the tables must be 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const RankWorkspace w = rank_carve(ws, max_users, n_k);
    RankKs k;
    k.n_k = n_k;
    for (int i = 0; i < RANK_MAX_KS; ++i) k.ks[i] = i < n_k ? ks[i] : 0;
    // every record starts as zeros with the "never written" flag: a slot that no append reached is counted by reduce, not summed as garbage
    PMGT_HIP(hipMemsetAsync(w.ndcg, 0, (size_t)((char*)w.flags - (char*)w.ndcg), st));
    PMGT_HIP(hipMemsetD32Async((hipDeviceptr_t)w.flags, (int)RANK_FLAG_UNWRITTEN, (size_t)w.capr, st));
    hipLaunchKernelGGL(rank_reset_kernel, dim3(1), dim3(64), 0, st, ws, max_users, k);
    const int max_k = ks[n_k - 1];
    for (int first = 0; first < max_k; first += RANK_TABLE_CHUNK) {
        RankTableChunk chunk;
        const int n = std::min(RANK_TABLE_CHUNK, max_k - first);
        for (int i = 0; i < RANK_TABLE_CHUNK; ++i) {
            chunk.disc[i] = i < n ? disc[first + i] : 0.0;
            chunk.idcg[i] = i < n ? idcg[first + i] : 0.0;
        }
        hipLaunchKernelGGL(rank_table_kernel, dim3(1), dim3(RANK_TABLE_CHUNK), 0, st, w.disc, w.idcg, first, n, chunk);
    }
    PMGT_LAUNCH_OK();
    return 0;
}

int pmgt_rank_append(void* ws, int64_t max_users, const float* logits, const float* labels, const int32_t* counts, int64_t row_stride,
                     int64_t user_offset, int64_t n_users, void* stream) {
    if (int rc = rank_check(ws, max_users, "pmgt_rank_append")) return rc;
    PMGT_CHECK(row_stride >= 1 && row_stride <= RANK_MAX_ROW, -2, "pmgt_rank_append: row_stride = %lld outside [1, %d]", (long long)row_stride,
               RANK_MAX_ROW);
    PMGT_CHECK(user_offset >= 0 && user_offset <= max_users && n_users >= 0 && n_users <= max_users - user_offset, -2,      // (no sum: no overflow)
               "pmgt_rank_append: %lld user slots from %lld do not fit max_users = %lld", (long long)n_users, (long long)user_offset,
               (long long)max_users);
    PMGT_CHECK(logits && labels, -2, "pmgt_rank_append: NULL logits or labels");
    PMGT_CHECK(((uintptr_t)logits & 3) == 0 && ((uintptr_t)labels & 3) == 0 && ((uintptr_t)counts & 3) == 0, -2,
               "pmgt_rank_append: logits, labels and counts must be 4-byte aligned");
    if (n_users == 0) return 0;
    hipLaunchKernelGGL(rank_append_kernel, dim3((unsigned)n_users), dim3(RANK_THREADS), 0, (hipStream_t)stream, ws, max_users, logits, labels, counts,
                       (int)row_stride, user_offset, (int)n_users);
    PMGT_LAUNCH_OK();
    return 0;
}

int pmgt_rank_reduce(void* ws, int64_t max_users, int64_t n_users, void* stream) {
    if (int rc = rank_check(ws, max_users, "pmgt_rank_reduce")) return rc;
    PMGT_CHECK(n_users >= 1 && n_users <= max_users, -2, "pmgt_rank_reduce: n_users = %lld outside [1, max_users = %lld]", (long long)n_users,
               (long long)max_users);
    hipLaunchKernelGGL(rank_reduce_kernel, dim3(2 * RANK_MAX_KS + 2), dim3(RANK_THREADS), 0, (hipStream_t)stream, ws, max_users, n_users);
    PMGT_LAUNCH_OK();
    return 0;
}

}  // extern "C"
