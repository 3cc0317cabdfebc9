// Validation loss and ROC AUC on the device (pmgt_eval_* of include/pmgt_capi.h; pmgt_op_eval_* of include/pmgt_ops.h): what
// `_validation_and_test_step` / `_valid_and_test_epoch_end` compute on the host (pmgt/pmgt/trainer.py:162-195: sigmoid(logits) and labels
// collected per batch, the batch loss weighted by its size, sklearn's roc_auc_score at the end), without a device-to-host copy per batch.
// Kept out of csrc/ for optimizer_step.hip's reason: the measured step launches nothing of this.
//
// append: one thread per prediction writes score, sort key and label bit to its slot; one lane adds (double)loss * n_targets to the fp64
//   accumulator -- a multiply and an add, each rounded once (no fused multiply-add), in batch order: the host loop's arithmetic.
// reduce: sort the keys with the label bit as payload, then the Mann-Whitney statistic in integers.  With N(j) = negatives at sorted
//   positions [0, j) and, for a positive with key k, lb / ub = first position with key >= k / > k (its tie group is [lb, ub)):
//       twoU = sum over tie groups of p (2 neg_below + q) = sum over positives of N(lb) + N(ub)
//   (a positive counts the negatives below its group twice and those inside it once).  lb / ub come from binary searches of the sorted
//   keys, N from a prefix table, so a tie group that spans tiles needs no special case.  Sums are uint64; across workgroups they meet in
//   one integer atomic per workgroup: the result does not depend on arrival order or launch geometry.
//   n <= EVAL_SMALL_MAX: ONE launch of one 1024-thread workgroup -- bitonic sort of the 33-bit composites (key << 1 | label) in LDS, prefix,
//     searches in LDS.  More: four 8-bit LSD radix passes (csrc/segsum.hip's scheme: per-tile digit histogram, column scan, stable scatter
//     by ballots + slot prefix) with the label byte as payload, per-tile negative counts, their scan, the prefix table, the searches.
// Sort stability: the LSD passes are stable by construction (they have to be); the order of equal keys in the result is irrelevant.
#include <algorithm>

#include "eval_metrics.h"

namespace pmgt {

// ---- append ------------------------------------------------------------------------------------------------------------------------------
template <bool FROM_LOGITS>
__global__ __launch_bounds__(256) void eval_append_kernel(const float* __restrict__ in, const float* __restrict__ labels, const float* __restrict__ loss,
                                                          int64_t offset, int n, double n_targets, uint32_t* __restrict__ keys,
                                                          float* __restrict__ scores, uint8_t* __restrict__ labs, double* __restrict__ acc,
                                                          unsigned long long* __restrict__ nan_count) {
#pragma clang fp contract(off)      // the product is rounded before the add, as on the host: hipcc would fuse the pair into one v_fmac_f64
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0 && loss != nullptr) {
        const double term = (double)loss[0] * n_targets;
        acc[0] = acc[0] + term;
    }
    if (i >= n) return;
    float s = in[i];
    if (FROM_LOGITS) s = 1.0f / (1.0f + expf(-s));      // accurate expf, IEEE divide
    const int64_t slot = offset + i;
    scores[slot] = s;
    labs[slot] = labels[i] != 0.f ? 1 : 0;
    if (s != s) {
        keys[slot] = 0xFFFFFFFFu;                        // not a key of any score: eval_key() of +Inf is 0xFF800000
        atomicAdd(nan_count, 1ull);
    } else {
        keys[slot] = eval_key(s);
    }
}

// ---- the statistic, shared by both paths ------------------------------------------------------------------------------------------------------
template <typename KeyAt> __device__ __forceinline__ int first_not_less(KeyAt key_at, int n, uint32_t k) {      // first i in [0, n] with key[i] >= k
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key_at(mid) < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}
template <typename KeyAt> __device__ __forceinline__ int first_greater(KeyAt key_at, int n, uint32_t k) {       // first i in [0, n] with key[i] > k
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (key_at(mid) <= k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ---- small path: one workgroup, everything in LDS -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(EVAL_SMALL_THREADS) void eval_reduce_small_kernel(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ labs, int n,
                                                                               int npad /* power of two, n <= npad <= EVAL_SMALL_MAX */,
                                                                               unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s[EVAL_SMALL_MAX];
    __shared__ uint32_t negpre[EVAL_SMALL_MAX];
    __shared__ uint32_t wtot[EVAL_SMALL_THREADS / 64];
    __shared__ unsigned long long wsum[EVAL_SMALL_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < npad; i += EVAL_SMALL_THREADS)
        s[i] = i < n ? (((unsigned long long)keys[i] << 1) | labs[i]) : ~0ull;      // padding sorts behind every composite (< 2^33)
    __syncthreads();
    for (int k = 2; k <= npad; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (npad >> 1); t += EVAL_SMALL_THREADS) {
                const int i = 2 * t - (t & (j - 1)), l = i + j;         // bit j of i clear, l = i | j: every pair once
                const bool up = (i & k) == 0;
                const unsigned long long a = s[i], b = s[l];
                if ((a > b) == up) { s[i] = b; s[l] = a; }
            }
            __syncthreads();
        }
    }
    // negpre[i] = negatives at sorted positions [0, i): thread t owns positions 4t .. 4t + 3
    constexpr int PER = EVAL_SMALL_MAX / EVAL_SMALL_THREADS;
    uint32_t c = 0;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const int i = tid * PER + e;
        c += (i < n && (s[i] & 1ull) == 0ull) ? 1u : 0u;
    }
    uint32_t inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    uint32_t run = inc - c, n_neg = 0;
    for (int w = 0; w < EVAL_SMALL_THREADS / 64; ++w) {
        if (w < wave) run += wtot[w];
        n_neg += wtot[w];
    }
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const int i = tid * PER + e;
        if (i < n) {
            negpre[i] = run;
            run += (s[i] & 1ull) == 0ull ? 1u : 0u;
        }
    }
    __syncthreads();
    auto key_at = [&](int i) { return (uint32_t)(s[i] >> 1); };
    auto neg_before = [&](int j) { return j >= n ? n_neg : negpre[j]; };
    unsigned long long sum = 0;
    for (int i = tid; i < n; i += EVAL_SMALL_THREADS) {
        if (s[i] & 1ull) {
            const uint32_t k = key_at(i);
            sum += (unsigned long long)neg_before(first_not_less(key_at, n, k)) + neg_before(first_greater(key_at, n, k));
        }
    }
    sum = wave_sum_u64(sum);
    if (lane == 0) wsum[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        unsigned long long tot = 0;
        for (int w = 0; w < EVAL_SMALL_THREADS / 64; ++w) tot += wsum[w];
        out[1] = tot;
        out[2] = (unsigned long long)n - n_neg;
        out[3] = n_neg;
        out[5] = (unsigned long long)n;
    }
}

// ---- multi-tile path: LSD radix sort (the scheme of csrc/segsum.hip, keys uint32 over all 32 bits, payload one label byte) ----------------------
__global__ __launch_bounds__(256) void eval_hist_kernel(const uint32_t* __restrict__ kin, int n, int shift, uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int base = blockIdx.x * EVAL_TILE;
#pragma unroll 4
    for (int j = 0; j < EVAL_ROUNDS; ++j) {
        const int idx = base + j * 256 + threadIdx.x;
        if (idx < n) atomicAdd(&h[(kin[idx] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(int64_t)blockIdx.x * 256 + threadIdx.x] = h[threadIdx.x];      // [tile][digit]
}

// column prefixes of the [tile][nb] table in place (wave = one column, lane = a strip of consecutive tiles), column totals to tot[nb]
__global__ __launch_bounds__(256) void eval_colscan_kernel(uint32_t* __restrict__ hist, int ntiles, uint32_t nb, uint32_t* __restrict__ tot) {
    const int lane = threadIdx.x & 63;
    const uint32_t dg = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (dg >= nb) return;                 // (wave-uniform)
    const int per = (ntiles + 63) / 64, t0 = min(ntiles, lane * per), t1 = min(ntiles, t0 + per);
    uint32_t s = 0;
    for (int t = t0; t < t1; ++t) s += hist[(int64_t)t * nb + dg];
    uint32_t inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    uint32_t run = inc - s;
    for (int t = t0; t < t1; ++t) {
        const uint32_t c = hist[(int64_t)t * nb + dg];
        hist[(int64_t)t * nb + dg] = run;
        run += c;
    }
    if (lane == 63) tot[dg] = inc;
}

// one counting pass: element of tile t with digit d goes to (keys with a smaller digit) + (digit d in earlier tiles) + (equals before it in the tile)
__global__ __launch_bounds__(256) void eval_scatter_kernel(const uint32_t* __restrict__ kin, const uint8_t* __restrict__ lin, int n, int shift,
                                                           const uint32_t* __restrict__ colpre /* [tile][digit] column prefixes */,
                                                           const uint32_t* __restrict__ coltot, uint32_t* __restrict__ kout, uint8_t* __restrict__ lout) {
    __shared__ uint16_t cnt[256][EVAL_SLOTS + 2];      // an odd number of dwords per row: the per-digit prefix walks rows conflict-free
    __shared__ uint32_t tbase[256];
    __shared__ uint32_t wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, tile = blockIdx.x;
    for (int i = tid; i < 256 * (EVAL_SLOTS + 2) / 2; i += 256) ((uint32_t*)cnt)[i] = 0u;
    {
        const uint32_t tot = coltot[tid], pre = colpre[(int64_t)tile * 256 + tid];
        uint32_t inc = tot;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane == 63) wtot[wave] = inc;
        __syncthreads();
        uint32_t woff = 0;
        for (int w = 0; w < wave; ++w) woff += wtot[w];
        tbase[tid] = woff + inc - tot + pre;
    }
    __syncthreads();
    uint32_t key[EVAL_ROUNDS], rank[EVAL_ROUNDS];
    uint8_t lab[EVAL_ROUNDS];
    const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
    for (int j = 0; j < EVAL_ROUNDS; ++j) {
        const int idx = tile * EVAL_TILE + j * 256 + wave * 64 + lane;
        const bool valid = idx < n;
        const int ic = valid ? idx : n - 1;
        key[j] = kin[ic];
        lab[j] = lin[ic];
        const uint32_t dg = (key[j] >> shift) & 255u;
        uint64_t m = __builtin_amdgcn_ballot_w64(valid);            // lanes holding the same digit as this one
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (dg >> b) & 1u;
            const uint64_t bal = __builtin_amdgcn_ballot_w64(bit);
            m &= bit ? bal : ~bal;
        }
        rank[j] = (uint32_t)__popcll(m & below);
        if (valid && rank[j] == 0) cnt[dg][j * 4 + wave] = (uint16_t)__popcll(m);
        if (!valid) rank[j] = 0xffffffffu;
    }
    __syncthreads();
    {   // exclusive prefix over the (round, wave) slots of digit `tid`
        uint32_t run = 0;
        for (int sidx = 0; sidx < EVAL_SLOTS; ++sidx) {
            const uint32_t c = cnt[tid][sidx];
            cnt[tid][sidx] = (uint16_t)run;
            run += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < EVAL_ROUNDS; ++j) {
        if (rank[j] != 0xffffffffu) {
            const uint32_t dg = (key[j] >> shift) & 255u;
            const uint32_t pos = tbase[dg] + cnt[dg][j * 4 + wave] + rank[j];
            if (pos < (uint32_t)n) {       // holds by construction (the table counts exactly these elements); never write outside the buffer
                kout[pos] = key[j];
                lout[pos] = lab[j];
            }
        }
    }
}

// negatives of every tile of the sorted order
__global__ __launch_bounds__(256) void eval_tile_neg_kernel(const uint8_t* __restrict__ labs, int n, uint32_t* __restrict__ tileneg) {
    __shared__ uint32_t w4[4];
    const int base = blockIdx.x * EVAL_TILE;
    uint32_t c = 0;
#pragma unroll
    for (int j = 0; j < EVAL_ROUNDS; ++j) {
        const int idx = base + j * 256 + threadIdx.x;
        c += (idx < n && labs[idx] == 0) ? 1u : 0u;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) w4[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) tileneg[blockIdx.x] = w4[0] + w4[1] + w4[2] + w4[3];
}

// one workgroup: tileneg [ntiles] -> exclusive prefixes in place, tileneg[ntiles] = total; header: twoU = 0, n_pos, n_neg, n
__global__ __launch_bounds__(256) void eval_tile_scan_kernel(uint32_t* __restrict__ tileneg, int ntiles, int n, unsigned long long* __restrict__ out) {
    __shared__ uint32_t wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = (ntiles + 255) / 256, t0 = min(ntiles, tid * per), t1 = min(ntiles, t0 + per);
    uint32_t s = 0;
    for (int t = t0; t < t1; ++t) s += tileneg[t];
    uint32_t inc = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    uint32_t run = inc - s, total = 0;
    for (int w = 0; w < 4; ++w) {
        if (w < wave) run += wtot[w];
        total += wtot[w];
    }
    for (int t = t0; t < t1; ++t) {
        const uint32_t c = tileneg[t];
        tileneg[t] = run;
        run += c;
    }
    if (tid == 0) {
        tileneg[ntiles] = total;
        out[1] = 0ull;
        out[2] = (unsigned long long)n - total;
        out[3] = total;
        out[5] = (unsigned long long)n;
    }
}

// negpre[i] = negatives at sorted positions [0, i), i < n: thread t of a tile owns its positions 8t .. 8t + 7
__global__ __launch_bounds__(256) void eval_neg_prefix_kernel(const uint8_t* __restrict__ labs, int n, const uint32_t* __restrict__ tileneg,
                                                              uint32_t* __restrict__ negpre) {
    __shared__ uint32_t wtot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int first = blockIdx.x * EVAL_TILE + tid * EVAL_ROUNDS;
    uint32_t c = 0;
#pragma unroll
    for (int e = 0; e < EVAL_ROUNDS; ++e) c += (first + e < n && labs[first + e] == 0) ? 1u : 0u;
    uint32_t inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    if (lane == 63) wtot[wave] = inc;
    __syncthreads();
    uint32_t run = tileneg[blockIdx.x] + inc - c;
    for (int w = 0; w < wave; ++w) run += wtot[w];
#pragma unroll
    for (int e = 0; e < EVAL_ROUNDS; ++e) {
        if (first + e < n) {
            negpre[first + e] = run;
            run += labs[first + e] == 0 ? 1u : 0u;
        }
    }
}

__global__ __launch_bounds__(256) void eval_stat_kernel(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ labs, int n,
                                                        const uint32_t* __restrict__ negpre, const uint32_t* __restrict__ n_neg_p,
                                                        unsigned long long* __restrict__ out) {
    __shared__ unsigned long long wsum[4];
    const uint32_t n_neg = n_neg_p[0];
    auto key_at = [&](int i) { return keys[i]; };
    auto neg_before = [&](int j) { return j >= n ? n_neg : negpre[j]; };
    unsigned long long sum = 0;
    const int base = blockIdx.x * EVAL_TILE;
    for (int j = 0; j < EVAL_ROUNDS; ++j) {
        const int i = base + j * 256 + threadIdx.x;
        if (i < n && labs[i] != 0) {
            const uint32_t k = keys[i];
            sum += (unsigned long long)neg_before(first_not_less(key_at, n, k)) + neg_before(first_greater(key_at, n, k));
        }
    }
    sum = wave_sum_u64(sum);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long tot = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (tot) atomicAdd(&out[1], tot);        // integer: order-independent
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------------
static int eval_check(const void* ws, int64_t capacity, const char* who) {
    PMGT_CHECK(ws != nullptr, -2, "%s: NULL workspace", who);
    PMGT_CHECK(capacity >= 1 && capacity <= EVAL_MAX_CAPACITY, -2, "%s: capacity = %lld outside [1, %lld]", who, (long long)capacity,
               (long long)EVAL_MAX_CAPACITY);
    PMGT_CHECK(((uintptr_t)ws & 15) == 0, -2, "%s: the workspace must be 16-byte aligned", who);
    return 0;
}

template <bool FROM_LOGITS>
static int eval_append(void* ws, int64_t capacity, const float* in, const float* labels, const float* loss, int64_t offset, int64_t n,
                       int64_t n_targets, hipStream_t st, const char* who) {
    if (int rc = eval_check(ws, capacity, who)) return rc;
    PMGT_CHECK(offset >= 0 && n >= 0 && offset + n <= capacity, -2, "%s: slots [%lld, %lld) do not fit the capacity of %lld", who, (long long)offset,
               (long long)(offset + n), (long long)capacity);
    PMGT_CHECK(n == 0 || (in && labels), -2, "%s: NULL input", who);
    PMGT_CHECK(n_targets >= 0, -2, "%s: n_targets = %lld is negative", who, (long long)n_targets);
    if (n == 0 && loss == nullptr) return 0;
    const EvalWorkspace w = eval_carve(ws, capacity);
    hipLaunchKernelGGL(eval_append_kernel<FROM_LOGITS>, dim3((unsigned)std::max<int64_t>(1, cdiv64(n, 256))), dim3(256), 0, st, in, labels, loss, offset, (int)n,
                       (double)n_targets, w.keys, w.scores, w.labels, w.acc, w.u + 4);
    PMGT_LAUNCH_OK();
    return 0;
}

}  // namespace pmgt

using namespace pmgt;

extern "C" {

int64_t pmgt_eval_workspace_bytes(int64_t capacity) {
    if (capacity < 1 || capacity > EVAL_MAX_CAPACITY) return -2;
    return eval_carve(nullptr, capacity).bytes;
}

int pmgt_eval_reset(void* ws, int64_t capacity, void* stream) {
    if (int rc = eval_check(ws, capacity, "pmgt_eval_reset")) return rc;
    PMGT_HIP(hipMemsetAsync(ws, 0, EVAL_HEADER_BYTES, (hipStream_t)stream));
    return 0;
}

int pmgt_eval_append(void* ws, int64_t capacity, const float* logits, const float* labels, const float* loss, int64_t offset, int64_t n,
                     int64_t n_targets, void* stream) {
    return eval_append<true>(ws, capacity, logits, labels, loss, offset, n, n_targets, (hipStream_t)stream, "pmgt_eval_append");
}

int pmgt_op_eval_append_scores(void* ws, int64_t capacity, const float* scores, const float* labels, const float* loss, int64_t offset, int64_t n,
                               int64_t n_targets, void* stream) {
    return eval_append<false>(ws, capacity, scores, labels, loss, offset, n, n_targets, (hipStream_t)stream, "pmgt_op_eval_append_scores");
}

int pmgt_op_eval_small_max(void) { return EVAL_SMALL_MAX; }

int pmgt_eval_reduce(void* ws, int64_t capacity, int64_t n, void* stream) {
    if (int rc = eval_check(ws, capacity, "pmgt_eval_reduce")) return rc;
    PMGT_CHECK(n >= 1 && n <= capacity, -2, "pmgt_eval_reduce: n = %lld outside [1, capacity = %lld]", (long long)n, (long long)capacity);
    const EvalWorkspace w = eval_carve(ws, capacity);
    hipStream_t st = (hipStream_t)stream;
    if (n <= EVAL_SMALL_MAX) {
        int npad = 2;
        while (npad < n) npad <<= 1;
        hipLaunchKernelGGL(eval_reduce_small_kernel, dim3(1), dim3(EVAL_SMALL_THREADS), 0, st, w.keys, w.labels, (int)n, npad, w.u);
        PMGT_LAUNCH_OK();
        return 0;
    }
    const int ni = (int)n, ntiles = eval_tiles(n);
    const uint32_t* kin = w.keys;
    const uint8_t* lin = w.labels;
    for (int p = 0; p < 4; ++p) {       // slots -> b -> c -> b -> c: the slot-order arrays stay as append left them
        uint32_t* kout = (p & 1) ? w.keys_c : w.keys_b;
        uint8_t* lout = (p & 1) ? w.labels_c : w.labels_b;
        hipLaunchKernelGGL(eval_hist_kernel, dim3(ntiles), dim3(256), 0, st, kin, ni, p * 8, w.hist);
        hipLaunchKernelGGL(eval_colscan_kernel, dim3(64), dim3(256), 0, st, w.hist, ntiles, 256u, w.coltot);
        hipLaunchKernelGGL(eval_scatter_kernel, dim3(ntiles), dim3(256), 0, st, kin, lin, ni, p * 8, w.hist, w.coltot, kout, lout);
        PMGT_LAUNCH_OK();
        kin = kout; lin = lout;
    }
    uint32_t* negpre = w.keys_b;         // the sorted order sits in (keys_c, labels_c)
    hipLaunchKernelGGL(eval_tile_neg_kernel, dim3(ntiles), dim3(256), 0, st, lin, ni, w.tileneg);
    hipLaunchKernelGGL(eval_tile_scan_kernel, dim3(1), dim3(256), 0, st, w.tileneg, ntiles, ni, w.u);
    hipLaunchKernelGGL(eval_neg_prefix_kernel, dim3(ntiles), dim3(256), 0, st, lin, ni, w.tileneg, negpre);
    hipLaunchKernelGGL(eval_stat_kernel, dim3(ntiles), dim3(256), 0, st, kin, lin, ni, negpre, w.tileneg + ntiles, w.u);
    PMGT_LAUNCH_OK();
    return 0;
}

}  // extern "C"
