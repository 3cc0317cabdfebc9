// Evaluation on the whole catalogue (pmgt_rank_heldout, pmgt_rank_heldout_reduce of include/pmgt_capi.h): for every held-out (user, item)
// pair the exact 1-based place of the item among the user's eligible items in the order of topk_rows.hip, and nDCG@k / Recall@k / HR@k /
// MRR from those places -- the reference's get_ndcg / get_recall (pmgt/metrics.py:16-37) on each user's whole-catalogue list, without
// building the list: a top-k is blind beyond k, a rank is not.  Kept out of csrc/ for eval_metrics.hip's reason: the measured step
// launches nothing of this.
//
// THE ORDER is that of pmgt_topk_rows: descending composite c(j) = key(j) << 32 | (0xFFFFFFFF - j), key = eval_key() of eval_metrics.h and
// 0xFFFFFFFF for a NaN; the composites of a row are distinct, so
//       rank(u, p) = 1 + #{ j eligible for u : c(j) > c(p) }
// has no tie to break.
//
// rank_heldout_kernel: one 256-thread workgroup per row, per chunk of up to 1 024 of the user's held-out items
//   sort      the chunk's composites go to LDS and are sorted descending by a bitonic network (padding 0: no composite is 0)
//   stream    the row is read once, coalesced; item j finds pos = #{sorted >= c(j)} by a binary search in LDS -- j is above exactly the
//             sorted entries from pos on -- and adds 1 to bin pos of an LDS histogram (the bin past the last entry is never needed)
//   exclude   the user's exclusion list is walked and every DISTINCT excluded item takes its 1 back the same way; an excluded item that is
//             in the sorted array marks that held-out item.  A list in non-decreasing order (what exclusion_csr builds) shows a duplicate
//             by its left neighbour; any other list is checked entry against every earlier entry: L^2 / 2 global reads by this one workgroup and
//             per chunk, right but slow for long lists -- the header tells the raw caller to sort them
//   scan      an inclusive prefix sum over the bins: entry i of the sorted array has scan[i] eligible items above it
//   write     every held-out item looks its composite up again and stores 1 + scan[i], or 0 when it is excluded
// NaNs are counted the same way (the row's minus the distinct excluded ones).  Integer LDS atomics only, whose sums do not depend on
// the order of the adds; no floating-point atomic, no workspace: the result is a pure function of the inputs.
//
// heldout_records_kernel: one wave per evaluated user; the ranks below max(ks) set a byte in a rank-indexed LDS array, which is then
//   walked in ascending rank as ranking_metrics.hip's append does: the discounts are added in the reference's order, one division per metric.
// heldout_sums_kernel: one workgroup per quantity, ranking_metrics.hip's fixed tree: thread t adds the users t, t + 256, ... in ascending
//   order, a shuffle tree over the lanes, the four wave sums in order.
#include "ranking_metrics.h"

namespace pmgt {

static constexpr int HELD_THREADS = 256, HELD_WAVES = HELD_THREADS / 64, HELD_CHUNK = PMGT_RANK_HELDOUT_CHUNK;
static constexpr int64_t HELD_MAX_ITEMS = 0x7FFFFFFELL;      // 2^31 - 2, as pmgt_topk_rows
static constexpr uint32_t HELD_NAN_KEY = 0xFFFFFFFFu;
static_assert(HELD_CHUNK == 4 * HELD_THREADS, "the scan gives every thread four bins");

struct HeldoutArgs {
    const float* scores;        // [n][row_stride]
    const int64_t* users;       // [n]
    const int64_t* indptr;      // [user_num + 1] or NULL
    const int32_t* excl;        // exclusion lists
    const int64_t* held_indptr; // [user_num + 1]
    const int32_t* held;        // held-out lists
    int32_t* ranks;             // [n_held]
    uint32_t* out_flags;        // [n]
    int64_t row_stride, user_num, n_excl, n_held;
    int n_items;
};

struct HeldoutKs {
    int n_k;
    int ks[RANK_MAX_KS];
};

__device__ __forceinline__ unsigned long long held_composite(float s, int64_t j) {
    const uint32_t key = s != s ? HELD_NAN_KEY : eval_key(s);
    return ((unsigned long long)key << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)j);
}

// #{ i < P : s[i] >= c } of a descending array whose length P is a power of two
__device__ __forceinline__ int held_count_ge(const unsigned long long* s, int P, unsigned long long c) {
    int pos = 0;
    for (int step = P >> 1; step > 0; step >>= 1)
        if (s[pos + step - 1] >= c) pos += step;
    return pos + (s[pos] >= c ? 1 : 0);
}

__global__ __launch_bounds__(HELD_THREADS) void rank_heldout_kernel(HeldoutArgs a) {
    __shared__ unsigned long long sorted[HELD_CHUNK];        // 8 KiB
    __shared__ uint32_t hist[HELD_CHUNK];                    // 4 KiB: bin i = items above exactly the entries i, i + 1, ...
    __shared__ uint8_t gone[HELD_CHUNK];                     // the held-out item at entry i is excluded
    __shared__ uint32_t wtot[HELD_WAVES];
    __shared__ int nan_s, unsorted_s, gone_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = blockIdx.x;
    const int I = a.n_items;
    const int64_t uid = a.users[row];
    if (uid < 0 || uid >= a.user_num) return;                // (uniform; the host surface refuses other ids)
    int64_t hlo = a.held_indptr[uid], hhi = a.held_indptr[uid + 1];
    hlo = hlo < 0 ? 0 : hlo;
    hhi = hhi > a.n_held ? a.n_held : hhi;
    if (hhi <= hlo) return;                                  // (uniform) no held-out item: nothing is written
    int64_t elo = 0, ehi = 0;
    if (a.indptr) {
        elo = a.indptr[uid];
        ehi = a.indptr[uid + 1];
        elo = elo < 0 ? 0 : elo;
        ehi = ehi > a.n_excl ? a.n_excl : ehi;
        if (ehi < elo) ehi = elo;
    }
    const float* __restrict__ x = a.scores + row * a.row_stride;
    if (tid == 0) { nan_s = 0; unsorted_s = 0; gone_s = 0; }
    __syncthreads();
    {
        bool bad = false;
        for (int64_t e = elo + 1 + tid; e < ehi; e += HELD_THREADS) bad |= a.excl[e - 1] > a.excl[e];
        if (bad) unsorted_s = 1;
    }
    __syncthreads();
    const bool in_order = unsorted_s == 0;
    for (int64_t h0 = hlo; h0 < hhi; h0 += HELD_CHUNK) {     // (uniform trip count)
        const int m = (int)((hhi - h0) < (int64_t)HELD_CHUNK ? (hhi - h0) : (int64_t)HELD_CHUNK);
        const bool first = h0 == hlo;                        // the NaNs are counted once
        int P = 1;
        while (P < m) P <<= 1;
        // ---- sort
        for (int t = tid; t < P; t += HELD_THREADS) {
            unsigned long long c = 0ull;                     // padding, and an item outside the row: sorts last, matches nothing
            if (t < m) {
                const int32_t p = a.held[h0 + t];
                if (p >= 0 && p < I) c = held_composite(x[p], p);
            }
            sorted[t] = c;
            hist[t] = 0u;
            gone[t] = 0;
        }
        __syncthreads();
        for (int size = 2; size <= P; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = tid; t < (P >> 1); t += HELD_THREADS) {
                    const int lo = ((t / stride) * stride << 1) + (t % stride), hi = lo + stride;
                    const bool desc = (lo & size) == 0;
                    const unsigned long long u = sorted[lo], v = sorted[hi];
                    if ((u < v) == desc) { sorted[lo] = v; sorted[hi] = u; }
                }
                __syncthreads();
            }
        // ---- stream
        int n_nan = 0;
#pragma unroll 4
        for (int64_t j = tid; j < I; j += HELD_THREADS) {
            const float s = x[j];
            n_nan += s != s ? 1 : 0;
            const int pos = held_count_ge(sorted, P, held_composite(s, j));
            if (pos < m) atomicAdd(&hist[pos], 1u);
        }
        if (first && n_nan) atomicAdd(&nan_s, n_nan);
        // ---- exclude
        for (int64_t e = elo + tid; e < ehi; e += HELD_THREADS) {
            const int32_t j = a.excl[e];
            if (j < 0 || j >= I) continue;
            bool dup = false;
            if (in_order) {
                dup = e > elo && a.excl[e - 1] == j;
            } else {
                for (int64_t f = elo; f < e && !dup; ++f) dup = a.excl[f] == j;
            }
            if (dup) continue;
            const float s = x[j];
            if (first && s != s) atomicSub(&nan_s, 1);
            const unsigned long long c = held_composite(s, j);
            const int pos = held_count_ge(sorted, P, c);
            if (pos > 0 && sorted[pos - 1] == c) gone[pos - 1] = 1;
            if (pos < m) atomicSub(&hist[pos], 1u);
        }
        __syncthreads();
        // ---- scan: inclusive prefix sums over the bins [0, P), four consecutive bins a thread
        {
            uint32_t v[4], sum = 0u;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                v[i] = 4 * tid + i < P ? hist[4 * tid + i] : 0u;
                sum += v[i];
            }
            uint32_t incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const uint32_t up = __shfl_up(incl, o, 64);
                if (lane >= o) incl += up;
            }
            if (lane == 63) wtot[wave] = incl;
            __syncthreads();
            uint32_t run = incl - sum;
            for (int w = 0; w < wave; ++w) run += wtot[w];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                run += v[i];
                if (4 * tid + i < P) hist[4 * tid + i] = run;
            }
        }
        __syncthreads();
        // ---- write
        bool any_gone = false;
        for (int t = tid; t < m; t += HELD_THREADS) {
            const int32_t p = a.held[h0 + t];
            int32_t rank = 0;
            if (p >= 0 && p < I) {
                const int at = held_count_ge(sorted, P, held_composite(x[p], p)) - 1;      // the (last) entry that holds c(p)
                if (at >= 0 && at < m) {
                    if (gone[at]) any_gone = true;
                    else rank = 1 + (int32_t)hist[at];
                }
            }
            a.ranks[h0 + t] = rank;
        }
        if (any_gone) gone_s = 1;
        __syncthreads();                                     // the next chunk overwrites the arrays
    }
    if (tid == 0) a.out_flags[row] = (nan_s > 0 ? PMGT_TOPK_FLAG_NAN : 0u) | (gone_s ? PMGT_RANK_HELDOUT_FLAG_EXCLUDED : 0u);
}

// ---- metrics: one wave per evaluated user -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void heldout_records_kernel(const int32_t* __restrict__ ranks, const int64_t* __restrict__ held_indptr,
                                                             const int64_t* __restrict__ users, int64_t n_users, int64_t user_num,
                                                             int64_t n_held, HeldoutKs ks, const double* __restrict__ disc,
                                                             const double* __restrict__ idcg, double* __restrict__ records) {
    __shared__ uint8_t hit[RANK_MAX_K];                      // hit[r] = a held-out item has rank r + 1
    const int lane = threadIdx.x;
    const int64_t i = blockIdx.x;
    const int n_k = ks.n_k, max_k = ks.ks[n_k - 1];
    for (int r = lane; r < max_k; r += 64) hit[r] = 0;
    __syncthreads();
    const int64_t uid = users[i];
    int64_t lo = 0, hi = 0;
    if (uid >= 0 && uid < user_num) {
        lo = held_indptr[uid];
        hi = held_indptr[uid + 1];
        lo = lo < 0 ? 0 : lo;
        hi = hi > n_held ? n_held : hi;
        if (hi < lo) hi = lo;
    }
    const int64_t n_pos = hi - lo;
    int best = 0x7FFFFFFF;
    for (int64_t h = lo + lane; h < hi; h += 64) {
        const int r = ranks[h];
        if (r >= 1) {
            best = min(best, r);
            if (r <= max_k) hit[r - 1] = 1;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) best = min(best, __shfl_xor(best, o, 64));
    __syncthreads();
    // every lane the same values: the hit ranks in ascending order, dcg and hits emitted where a cut-off is passed
    double dcg = 0.0;
    int hits = 0, ki = 0;
    for (int base = 0; base < max_k; base += 64) {
        const int r = base + lane;
        unsigned long long m = __builtin_amdgcn_ballot_w64(r < max_k && hit[r] != 0);
        while (ki < n_k && ks.ks[ki] <= base + 64) {
            const int k = ks.ks[ki], kb = k - base;          // 1 .. 64: ranks base .. base + kb - 1 are below this cut-off
            const unsigned long long below = kb >= 64 ? ~0ull : ((1ull << kb) - 1ull);
            unsigned long long take = m & below;
            m &= ~below;
            while (take) {
                dcg = dcg + disc[base + __builtin_ctzll(take)];
                ++hits;
                take &= take - 1ull;
            }
            if (lane == 0) {
                const bool some = n_pos > 0;
                records[(int64_t)ki * n_users + i] = some ? dcg / idcg[(n_pos < (int64_t)k ? (int)n_pos : k) - 1] : 0.0;
                records[(int64_t)(n_k + ki) * n_users + i] = some ? (double)hits / (double)n_pos : 0.0;
                records[(int64_t)(2 * n_k + ki) * n_users + i] = best <= k ? 1.0 : 0.0;
            }
            ++ki;
        }
        while (m) {
            dcg = dcg + disc[base + __builtin_ctzll(m)];
            ++hits;
            m &= m - 1ull;
        }
    }
    if (lane == 0) records[(int64_t)(3 * n_k) * n_users + i] = best != 0x7FFFFFFF ? 1.0 / (double)best : 0.0;
}

// workgroup q < 3 n_k + 1 sums row q of the records in a fixed order; workgroup 3 n_k + 1 counts the flags
__global__ __launch_bounds__(HELD_THREADS) void heldout_sums_kernel(const double* __restrict__ records, const uint32_t* __restrict__ flags,
                                                                    int64_t n, int n_k, double* __restrict__ header) {
    __shared__ double wsum[HELD_WAVES];
    __shared__ unsigned long long wcnt[HELD_WAVES][2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = blockIdx.x;
    if (q == 3 * n_k + 1) {
        unsigned long long n_nan = 0, n_gone = 0;
        if (flags)
            for (int64_t u = tid; u < n; u += HELD_THREADS) {
                const uint32_t f = flags[u];
                n_nan += (f & PMGT_TOPK_FLAG_NAN) ? 1ull : 0ull;
                n_gone += (f & PMGT_RANK_HELDOUT_FLAG_EXCLUDED) ? 1ull : 0ull;
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            n_nan += __shfl_xor(n_nan, o, 64);
            n_gone += __shfl_xor(n_gone, o, 64);
        }
        if (lane == 0) { wcnt[wave][0] = n_nan; wcnt[wave][1] = n_gone; }
        __syncthreads();
        if (tid == 0) {
            unsigned long long* u = (unsigned long long*)header;
            u[13] = (unsigned long long)n;
            u[14] = wcnt[0][0] + wcnt[1][0] + wcnt[2][0] + wcnt[3][0];
            u[15] = wcnt[0][1] + wcnt[1][1] + wcnt[2][1] + wcnt[3][1];
            for (int g = 0; g < 3; ++g)
                for (int i = n_k; i < RANK_MAX_KS; ++i) header[g * RANK_MAX_KS + i] = 0.0;      // the cut-offs this call does not have
        }
        return;
    }
    if (q > 3 * n_k) return;
    const double* src = records + (int64_t)q * n;
    double s = 0.0;
    for (int64_t u = tid; u < n; u += HELD_THREADS) s = s + src[u];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = s + __shfl_xor(s, o, 64);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    if (tid == 0) header[q == 3 * n_k ? 3 * RANK_MAX_KS : (q / n_k) * RANK_MAX_KS + q % n_k] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

}  // namespace pmgt

using namespace pmgt;

extern "C" {

int pmgt_rank_heldout(const float* scores, int64_t row_stride, int64_t n, int64_t n_items, const int64_t* users, const int64_t* indptr,
                      const int32_t* excluded, int64_t user_num, int64_t n_excluded, const int64_t* held_indptr, const int32_t* held_items,
                      int64_t n_heldout, int32_t* ranks, uint32_t* out_flags, void* stream) {
    PMGT_CHECK(n_items >= 1 && n_items <= HELD_MAX_ITEMS, -2, "pmgt_rank_heldout: %lld items outside [1, 2^31 - 2]", (long long)n_items);
    PMGT_CHECK(n >= 1 && n <= 0x7FFFFFFFLL, -2, "pmgt_rank_heldout: n = %lld rows outside [1, 2^31 - 1]", (long long)n);
    PMGT_CHECK(row_stride >= n_items, -2, "pmgt_rank_heldout: row_stride = %lld below the %lld items", (long long)row_stride, (long long)n_items);
    PMGT_CHECK(scores && users && held_indptr && ranks && out_flags, -2, "pmgt_rank_heldout: NULL buffer");
    PMGT_CHECK((((uintptr_t)scores | (uintptr_t)ranks | (uintptr_t)out_flags | (uintptr_t)excluded | (uintptr_t)held_items) & 3) == 0 &&
               (((uintptr_t)users | (uintptr_t)indptr | (uintptr_t)held_indptr) & 7) == 0, -2, "pmgt_rank_heldout: misaligned buffer");
    PMGT_CHECK(user_num >= 1 && n_heldout >= 0 && (held_items != nullptr || n_heldout == 0), -2,
               "pmgt_rank_heldout: the held-out CSR needs user_num >= 1 and its item array");
    if (indptr) {
        PMGT_CHECK(n_excluded >= 0 && (excluded != nullptr || n_excluded == 0), -2, "pmgt_rank_heldout: an exclusion CSR needs its item array");
    }
    HeldoutArgs a;
    a.scores = scores;
    a.users = users;
    a.indptr = indptr;
    a.excl = excluded;
    a.held_indptr = held_indptr;
    a.held = held_items;
    a.ranks = ranks;
    a.out_flags = out_flags;
    a.row_stride = row_stride;
    a.user_num = user_num;
    a.n_excl = indptr ? n_excluded : 0;
    a.n_held = n_heldout;
    a.n_items = (int)n_items;
    hipLaunchKernelGGL(rank_heldout_kernel, dim3((unsigned)n), dim3(HELD_THREADS), 0, (hipStream_t)stream, a);
    PMGT_LAUNCH_OK();
    return 0;
}

int pmgt_rank_heldout_reduce(const int32_t* ranks, const int64_t* held_indptr, const int64_t* users, const uint32_t* flags, int64_t n_users,
                             int64_t user_num, int64_t n_heldout, const int* ks, int n_k, const double* disc, const double* idcg,
                             double* records, void* header, void* stream) {
    PMGT_CHECK(n_k >= 1 && n_k <= RANK_MAX_KS && ks != nullptr, -2, "pmgt_rank_heldout_reduce: n_k = %d outside [1, %d] or NULL ks", n_k, RANK_MAX_KS);
    HeldoutKs k;
    k.n_k = n_k;
    int prev = 0;
    for (int i = 0; i < RANK_MAX_KS; ++i) {
        k.ks[i] = i < n_k ? ks[i] : 0;
        if (i < n_k) {
            PMGT_CHECK(ks[i] > prev && ks[i] <= RANK_MAX_K, -2,
                       "pmgt_rank_heldout_reduce: ks[%d] = %d: the cut-offs must be strictly increasing in [1, %d]", i, ks[i], RANK_MAX_K);
            prev = ks[i];
        }
    }
    PMGT_CHECK(n_users >= 1 && n_users <= 0x7FFFFFFFLL, -2, "pmgt_rank_heldout_reduce: n_users = %lld outside [1, 2^31 - 1]", (long long)n_users);
    PMGT_CHECK(user_num >= 1 && n_heldout >= 1, -2, "pmgt_rank_heldout_reduce: user_num = %lld and n_heldout = %lld must be >= 1",
               (long long)user_num, (long long)n_heldout);
    PMGT_CHECK(ranks && held_indptr && users && disc && idcg && records && header, -2, "pmgt_rank_heldout_reduce: NULL buffer");
    PMGT_CHECK((((uintptr_t)ranks | (uintptr_t)flags) & 3) == 0 &&
               (((uintptr_t)held_indptr | (uintptr_t)users | (uintptr_t)disc | (uintptr_t)idcg | (uintptr_t)records | (uintptr_t)header) & 7) == 0,
               -2, "pmgt_rank_heldout_reduce: misaligned buffer");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(heldout_records_kernel, dim3((unsigned)n_users), dim3(64), 0, st, ranks, held_indptr, users, n_users, user_num, n_heldout, k,
                       disc, idcg, records);
    hipLaunchKernelGGL(heldout_sums_kernel, dim3(3 * n_k + 2), dim3(HELD_THREADS), 0, st, (const double*)records, flags, n_users, n_k,
                       (double*)header);
    PMGT_LAUNCH_OK();
    return 0;
}

}  // extern "C"
