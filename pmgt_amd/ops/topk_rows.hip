// The k best eligible items of every row of a score matrix, in the project's order (pmgt_topk_rows of include/pmgt_capi.h): what
// `pred.topk(100)` of the reference's test step (pmgt/ncf/trainer.py:202-219) does for one sampled candidate list, for whole catalogue rows
// with the user's known items left out.  Kept out of csrc/ for eval_metrics.hip's reason: the measured step launches nothing of this.
//
// THE ORDER is that of pmgt_rank_*: key = eval_key() of eval_metrics.h (a NaN score gets 0xFFFFFFFF and ranks first), descending, and among
// equal keys THE LOWER ITEM INDEX FIRST.  Both are one comparison on the 64-bit composite
//       c(j) = key(j) << 32 | (0xFFFFFFFF - j)
// which is distinct for every item of a row: the k best items are the k largest composites, and there are no ties left to break.
//
// One workgroup per row, four phases over the row's key image in the workspace (uint32 [n][I]):
//   keys      key(j) of every live entry; entries [I, row_stride) of the scores are never read
//   exclude   key 0 over the entries of the user's exclusion list -- no score has key 0 (eval_key(-inf) = 0x007FFFFF is the smallest), so
//             "key != 0" is "eligible"; every writer stores the same 0, duplicates in a list are harmless
//   select    radix-select of the kk-th largest composite, kk = min(k, eligible): up to eight 8-bit histogram passes from the top digit, each
//             narrowing to the bin that holds the kk-th; it stops as soon as the WHOLE bin is needed (continuous scores: after two or three
//             passes; the index digits are only walked when the k-th place falls inside a run of equal keys)
//   sort      the kk composites at or above the threshold are collected in LDS (their places there come from an integer counter and do not
//             matter) and sorted by a bitonic network: descending composite = the project's order
// The histograms are integer LDS atomics (counts do not depend on the order of the adds); no floating-point atomic anywhere: the result is a
// pure function of the inputs.
#include "eval_metrics.h"

namespace pmgt {

static constexpr int TOPK_THREADS = 256, TOPK_MAX_K = PMGT_TOPK_MAX_K;
static constexpr int64_t TOPK_MAX_ITEMS = 0x7FFFFFFELL;      // 2^31 - 2: item indices and the padding -1 fit an int32

struct TopkArgs {
    const float* scores;        // [n][row_stride]
    const int64_t* users;       // [n] or NULL
    const int64_t* indptr;      // [user_num + 1] or NULL
    const int32_t* excl;        // exclusion lists
    uint32_t* keys;             // workspace [n][I]
    int32_t* out_items;         // [n][k]
    float* out_scores;          // [n][k]
    uint32_t* out_flags;        // [n]
    int64_t row_stride, user_num, n_excl;
    int n_items, k;
};

__device__ __forceinline__ unsigned long long topk_composite(uint32_t key, int64_t j) {
    return ((unsigned long long)key << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)j);
}

__global__ __launch_bounds__(TOPK_THREADS) void topk_rows_kernel(TopkArgs a) {
    __shared__ uint32_t hist[256];
    __shared__ unsigned long long buf[TOPK_MAX_K];           // 8 KiB
    __shared__ int sel_bin, sel_above, sel_cnt, total_s, n_out, nan_s;
    const int tid = threadIdx.x, lane = tid & 63;
    const int64_t row = blockIdx.x;
    const int I = a.n_items, k = a.k;
    const float* __restrict__ x = a.scores + row * a.row_stride;
    uint32_t* keys = a.keys + row * (int64_t)I;
    if (tid == 0) { n_out = 0; nan_s = 0; }
    // ---- keys
    for (int64_t j = tid; j < I; j += TOPK_THREADS) {
        const float s = x[j];
        keys[j] = s != s ? 0xFFFFFFFFu : eval_key(s);
    }
    __syncthreads();
    // ---- exclude
    if (a.indptr) {
        const int64_t uid = a.users[row];
        if (uid >= 0 && uid < a.user_num) {                  // (the host surface refuses other ids; never read outside the lists)
            int64_t lo = a.indptr[uid], hi = a.indptr[uid + 1];
            lo = lo < 0 ? 0 : lo;
            hi = hi > a.n_excl ? a.n_excl : hi;
            for (int64_t e = lo + tid; e < hi; e += TOPK_THREADS) {
                const int32_t j = a.excl[e];
                if (j >= 0 && j < I) keys[j] = 0u;
            }
        }
        __syncthreads();
    }
    // ---- select
    unsigned long long prefix = 0ull;        // the digits fixed so far, the others zero
    int need = 0, kk = 0;
    bool any_nan = false;
    for (int pass = 0; pass < 8; ++pass) {
        const int shift = 56 - 8 * pass;
        hist[tid] = 0u;                      // (TOPK_THREADS == 256 bins)
        __syncthreads();
        for (int64_t j = tid; j < I; j += TOPK_THREADS) {
            const uint32_t key = keys[j];
            if (key == 0u) continue;
            if (pass == 0) any_nan |= key == 0xFFFFFFFFu;
            const unsigned long long c = topk_composite(key, j);
            if (pass == 0 || (c >> (shift + 8)) == (prefix >> (shift + 8))) atomicAdd(&hist[(unsigned)(c >> shift) & 255u], 1u);
        }
        if (pass == 0 && any_nan) nan_s = 1;
        __syncthreads();
        if (tid < 64) {
            // lane L owns the bins 255 - 4 L .. 252 - 4 L; an inclusive scan over the lanes gives the count above each
            uint32_t hb[4];
            uint32_t s = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) { hb[i] = hist[255 - 4 * lane - i]; s += hb[i]; }
            uint32_t incl = s;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t v = __shfl_up(incl, o, 64);
                if (lane >= o) incl += v;
            }
            int nd = need;
            if (pass == 0) {
                const int total = (int)__shfl(incl, 63, 64);
                nd = min(k, total);
                if (lane == 0) total_s = total;
            }
            uint32_t running = incl - s;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (nd > 0 && running < (uint32_t)nd && running + hb[i] >= (uint32_t)nd) {      // exactly one (lane, i)
                    sel_bin = 255 - 4 * lane - i;
                    sel_above = (int)running;
                    sel_cnt = (int)hb[i];
                }
                running += hb[i];
            }
        }
        __syncthreads();
        if (pass == 0) {
            kk = min(k, total_s);
            need = kk;
        }
        if (kk == 0) break;                                  // (uniform) nothing eligible
        prefix |= (unsigned long long)sel_bin << shift;
        need -= sel_above;
        if (sel_cnt == need) break;                          // (uniform) the whole bin is taken: everything at or above `prefix`
    }
    // ---- collect and sort
    int P = 1;
    while (P < kk) P <<= 1;
    if (kk > 0) {
        for (int64_t j = tid; j < I; j += TOPK_THREADS) {
            const uint32_t key = keys[j];
            if (key == 0u) continue;
            const unsigned long long c = topk_composite(key, j);
            if (c >= prefix) {
                const int at = atomicAdd(&n_out, 1);
                if (at < TOPK_MAX_K) buf[at] = c;
            }
        }
        for (int s = kk + tid; s < P; s += TOPK_THREADS) buf[s] = 0ull;      // padding sorts last (no composite is 0)
        __syncthreads();
        for (int size = 2; size <= P; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < (P >> 1); t += TOPK_THREADS) {
                    const int lo = ((t / stride) * stride << 1) + (t % stride), hi = lo + stride;
                    const bool desc = (lo & size) == 0;
                    const unsigned long long u = buf[lo], v = buf[hi];
                    if ((u < v) == desc) { buf[lo] = v; buf[hi] = u; }
                }
                __syncthreads();
            }
    }
    int32_t* oi = a.out_items + row * (int64_t)k;
    float* os = a.out_scores + row * (int64_t)k;
    for (int s = tid; s < k; s += TOPK_THREADS) {
        if (s < kk) {
            const int j = (int)(0xFFFFFFFFu - (uint32_t)(buf[s] & 0xFFFFFFFFull));
            const bool ok = j >= 0 && j < I;                 // (always: the kk slots hold composites of this row)
            oi[s] = ok ? j : -1;
            os[s] = ok ? x[j] : -__builtin_inff();           // the score as it came in, bit for bit
        } else {
            oi[s] = -1;
            os[s] = -__builtin_inff();
        }
    }
    if (tid == 0) a.out_flags[row] = (nan_s ? PMGT_TOPK_FLAG_NAN : 0u) | (total_s < k ? PMGT_TOPK_FLAG_SHORT : 0u);
}

}  // namespace pmgt

using namespace pmgt;

extern "C" {

int64_t pmgt_topk_workspace_bytes(int64_t n, int64_t n_items) {
    if (n < 1 || n > 0x7FFFFFFFLL || n_items < 1 || n_items > TOPK_MAX_ITEMS) return -2;
    if (n > (INT64_MAX / 4 - 16) / n_items) return -2;
    return (n * n_items * 4 + 15) / 16 * 16;
}

int pmgt_topk_rows(const float* scores, int64_t row_stride, int64_t n, int64_t n_items, int k, const int64_t* users, const int64_t* indptr,
                   const int32_t* excluded, int64_t user_num, int64_t n_excluded, void* workspace, int32_t* out_items, float* out_scores,
                   uint32_t* out_flags, void* stream) {
    PMGT_CHECK(k >= 1 && k <= TOPK_MAX_K, -2, "pmgt_topk_rows: k = %d outside [1, %d]", k, TOPK_MAX_K);
    PMGT_CHECK(n_items >= 1 && n_items <= TOPK_MAX_ITEMS, -2, "pmgt_topk_rows: %lld items outside [1, 2^31 - 2]", (long long)n_items);
    PMGT_CHECK(n >= 1 && n <= 0x7FFFFFFFLL, -2, "pmgt_topk_rows: n = %lld rows outside [1, 2^31 - 1]", (long long)n);
    PMGT_CHECK(pmgt_topk_workspace_bytes(n, n_items) > 0, -2, "pmgt_topk_rows: %lld x %lld keys do not fit an int64 byte count", (long long)n,
               (long long)n_items);
    PMGT_CHECK(row_stride >= n_items, -2, "pmgt_topk_rows: row_stride = %lld below the %lld items", (long long)row_stride, (long long)n_items);
    PMGT_CHECK(scores && workspace && out_items && out_scores && out_flags, -2, "pmgt_topk_rows: NULL buffer");
    PMGT_CHECK((((uintptr_t)scores | (uintptr_t)workspace | (uintptr_t)out_items | (uintptr_t)out_scores | (uintptr_t)out_flags |
                 (uintptr_t)excluded) & 3) == 0 && (((uintptr_t)users | (uintptr_t)indptr) & 7) == 0 && ((uintptr_t)workspace & 15) == 0, -2,
               "pmgt_topk_rows: misaligned buffer");
    if (indptr) {
        PMGT_CHECK(users != nullptr && user_num >= 1 && n_excluded >= 0 && (excluded != nullptr || n_excluded == 0), -2,
                   "pmgt_topk_rows: an exclusion CSR needs users, user_num >= 1 and its item array");
    }
    TopkArgs a;
    a.scores = scores;
    a.users = users;
    a.indptr = indptr;
    a.excl = excluded;
    a.keys = (uint32_t*)workspace;
    a.out_items = out_items;
    a.out_scores = out_scores;
    a.out_flags = out_flags;
    a.row_stride = row_stride;
    a.user_num = user_num;
    a.n_excl = n_excluded;
    a.n_items = (int)n_items;
    a.k = k;
    hipLaunchKernelGGL(topk_rows_kernel, dim3((unsigned)n), dim3(TOPK_THREADS), 0, (hipStream_t)stream, a);
    PMGT_LAUNCH_OK();
    return 0;
}

}  // extern "C"
