// Truncated, weighted item-kNN scoring of users from their histories over a PRECOMPUTED neighbour index (pmgt_knn_score of
// include/pmgt_capi.h): the index holds, per item i, its m best other items nbr[i][0 .. m) with their similarities sim[i][0 .. m); a
// candidate j is scored by the sum, over the history items that LIST it, of their (weighted) similarity to it.  Gather, LDS and store work:
// no MFMA, nothing of the table is read -- a user costs |H| m gathered entries and the I floats of the output row, whatever d was.  Kept out
// of csrc/ for ncf_score.hip's reason: the measured step launches nothing of this.
//
// THE SCORE.  With i_0 < i_1 < .. the items of the user's list IN THE ORDER OF THE LIST and w_t the weight of entry t (1 without weights):
//   acc = +0.0f;  for t = 0 .. len - 1:  if j is at slot c < m of row i_t:  acc = acc + term,  term = sim[i_t][c] (no weights) or
//   w_t * sim[i_t][c] rounded once to fp32; every sum rounded to fp32, none contracted into an fma.  scores[r][j] = acc.
// An item nobody lists scores +0.0 and a zero result is always +0.0 (the sum starts there).
//
// TILE.  A workgroup of 4 waves owns ONE batch slot and KNN_T = 8192 consecutive candidates, their accumulators in 32 KiB of LDS (five
// workgroups a CU).  Wave w owns the columns [2048 w, 2048 (w + 1)) of the tile: it zeroes them, then walks ALL the user's entries itself
// from the first to the last, an index row 64 slots at a time (coalesced 256-byte reads of nbr and sim), and each lane whose neighbour
// falls into the wave's columns does acc[j - j0] += term: a plain ds_read, add, ds_write.  That is race-free and ordered without a barrier
// or an atomic because (1) the live ids of one index row are pairwise distinct (THE CALLER CHECKS the index), so the lanes of one step hit
// distinct addresses, and (2) a column is only ever touched by one wave, in program order -- the order of the list and nothing else.  So the
// bits of scores[r][j] depend on H(u), its weights and the index rows of its items alone: not on n, the slot, the other users of the call,
// how the catalogue is cut into tiles or the launch geometry.  KNN_STEPS = 4 steps' global loads are issued before their LDS updates.
// After ONE barrier the workgroup stores the tile: 16-byte stores from the first 16-byte aligned address of the row's share on (ds_read_b128
// where the tile's first column is itself aligned, which a row_stride that is a multiple of 4 makes every row), single floats before and
// after.
// A slot past n is not stored, nor a column past n_items.  A user id outside [0, user_num) or an empty list is never dereferenced: its
// row is NaN.  A history item outside [0, n_items) is never dereferenced: it makes the whole row NaN.  A neighbour id < 0 (the padding of a
// short row) or >= n_items is skipped.  Offsets are 64-bit.  No atomics anywhere.
#include "ncf_head.h"

namespace pmgt {

static constexpr int KNN_T = 8192;                           // the candidates of a tile: 32 KiB of accumulators
static constexpr int KNN_THREADS = 256, KNN_WAVES = KNN_THREADS / 64, KNN_SUB = KNN_T / KNN_WAVES, KNN_STEPS = 4;
static constexpr int KNN_MAX_M = 1024;                       // PMGT_TOPK_MAX_K: what the index builder selects at most
static_assert(KNN_T % (4 * KNN_THREADS) == 0 && KNN_SUB % (4 * 64) == 0, "16-byte LDS accesses tile the wave's columns");

using knn_f4 = float __attribute__((ext_vector_type(4)));

struct KnnArgs {
    const int32_t* nbr;        // [n_items][idx_stride]
    const float* sim;          // [n_items][idx_stride]
    const int64_t* hist_ptr;   // [user_num + 1]
    const int32_t* hist_items;
    const float* hist_weights; // aligned with hist_items, or NULL
    const int64_t* users;      // [n]
    float* scores;             // [n][row_stride]
    int64_t idx_stride, row_stride, user_num;
    int n, n_items, m, item_tiles;
};

template <bool WEIGHTED> __global__ __launch_bounds__(KNN_THREADS) void knn_score_kernel(KnnArgs a) {
    __shared__ __attribute__((aligned(16))) float acc[KNN_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t j0 = (int64_t)(blockIdx.x % (unsigned)a.item_tiles) * KNN_T;
    const int r = (int)(blockIdx.x / (unsigned)a.item_tiles);
    const int width = (int)min((int64_t)KNN_T, (int64_t)a.n_items - j0);      // the live columns of the tile (>= 1)
    const int64_t u = a.users[r];
    int64_t start = 0, len = 0;
    if (u >= 0 && u < a.user_num) {
        start = a.hist_ptr[u];
        len = a.hist_ptr[u + 1] - start;
    }
    bool bad = len <= 0;                                     // the row is NaN (uniform over the workgroup: every wave walks the same list)
    if (!bad) {
        float* const mine = acc + wave * KNN_SUB;            // this wave's columns: zeroed, then updated, by this wave alone
#pragma unroll
        for (int i = 0; i < KNN_SUB / (4 * 64); ++i) *reinterpret_cast<knn_f4*>(mine + 4 * (lane + 64 * i)) = knn_f4{0.f, 0.f, 0.f, 0.f};
        const int64_t wlo = j0 + wave * KNN_SUB;             // its first candidate, and how many of them are live
        const int64_t wcount = min((int64_t)KNN_SUB, (int64_t)a.n_items - wlo);
        const int chunks = (a.m + 63) >> 6;
        int64_t t = 0;                                       // a step = (entry t, slots 64 c .. 64 c + 63), c the fastest
        int c = 0;
        while (t < len) {
            int32_t id[KNN_STEPS];
            float term[KNN_STEPS];
#pragma unroll
            for (int s = 0; s < KNN_STEPS; ++s) {
                id[s] = -1, term[s] = 0.f;
                if (t < len) {
                    const int slot = c * 64 + lane;
                    const int32_t item = a.hist_items[start + t];
                    if (item < 0 || item >= a.n_items) {
                        bad = true;
                    } else if (slot < a.m) {
                        const int64_t at = (int64_t)item * a.idx_stride + slot;
                        id[s] = a.nbr[at];
                        term[s] = a.sim[at];
                        if constexpr (WEIGHTED) term[s] = __fmul_rn(a.hist_weights[start + t], term[s]);
                    }
                    if (++c == chunks) c = 0, ++t;
                }
            }
            if (bad) break;
#pragma unroll
            for (int s = 0; s < KNN_STEPS; ++s) {            // in the order of the list: a column's sums are this wave's, one after the other
                const int64_t rel = (int64_t)id[s] - wlo;
                if (rel >= 0 && rel < wcount) mine[rel] = __fadd_rn(mine[rel], term[s]);
            }
        }
    }
    if (bad) {                                               // (uniform over the workgroup) every wave fills its own columns
#pragma unroll
        for (int i = 0; i < KNN_SUB / (4 * 64); ++i) {
            const float nan = __builtin_nanf("");
            *reinterpret_cast<knn_f4*>(acc + wave * KNN_SUB + 4 * (lane + 64 * i)) = knn_f4{nan, nan, nan, nan};
        }
    }
    __syncthreads();
    // the store: columns [0, width) of the tile to scores[r][j0 ..], 16-byte stores from the first aligned address on
    float* const dst = a.scores + (int64_t)r * a.row_stride + j0;
    const int head = min(width, (int)((4 - (((uintptr_t)dst >> 2) & 3)) & 3));
    const int body = (width - head) >> 2;
    if (tid < head) dst[tid] = acc[tid];
    if (head == 0) {
#pragma unroll 4
        for (int e = tid; e < body; e += KNN_THREADS) *reinterpret_cast<knn_f4*>(dst + 4 * e) = *reinterpret_cast<const knn_f4*>(acc + 4 * e);
    } else {
        for (int e = tid; e < body; e += KNN_THREADS) {
            const float* src = acc + head + 4 * e;
            *reinterpret_cast<knn_f4*>(dst + head + 4 * e) = knn_f4{src[0], src[1], src[2], src[3]};
        }
    }
    const int tail = head + 4 * body + tid;
    if (tail < width) dst[tail] = acc[tail];
}

}  // namespace pmgt

using namespace pmgt;

extern "C" int pmgt_knn_score_tile(void) { return KNN_T; }

extern "C" int pmgt_knn_score(const int32_t* nbr, const float* sim, int64_t idx_stride, int m, const int64_t* hist_ptr,
                              const int32_t* hist_items, const float* hist_weights, const int64_t* users, int64_t n, int64_t user_num,
                              int64_t n_items, float* scores, int64_t row_stride, void* stream) {
    PMGT_CHECK(m >= 1 && m <= KNN_MAX_M, -2, "pmgt_knn_score: m = %d outside [1, %d]", m, KNN_MAX_M);
    PMGT_CHECK(idx_stride >= m, -2, "pmgt_knn_score: idx_stride = %lld below m = %d", (long long)idx_stride, m);
    PMGT_CHECK(n >= 1 && n <= PMGT_NCF_MAX_USERS, -2, "pmgt_knn_score: n = %lld users outside [1, %d]", (long long)n, PMGT_NCF_MAX_USERS);
    PMGT_CHECK(n_items >= 1 && n_items <= 0x7FFFFFFELL, -2, "pmgt_knn_score: %lld items outside [1, 2^31 - 2]", (long long)n_items);
    PMGT_CHECK(user_num >= 1, -2, "pmgt_knn_score: user_num = %lld below 1", (long long)user_num);
    PMGT_CHECK(row_stride >= n_items, -2, "pmgt_knn_score: row_stride = %lld below the %lld items", (long long)row_stride, (long long)n_items);
    PMGT_CHECK(nbr && sim && hist_ptr && hist_items && users && scores, -2, "pmgt_knn_score: NULL buffer");
    PMGT_CHECK((((uintptr_t)nbr | (uintptr_t)sim | (uintptr_t)hist_items | (uintptr_t)hist_weights | (uintptr_t)scores) & 3) == 0
                   && (((uintptr_t)users | (uintptr_t)hist_ptr) & 7) == 0,
               -2, "pmgt_knn_score: misaligned buffer");
    KnnArgs a;
    a.nbr = nbr;
    a.sim = sim;
    a.hist_ptr = hist_ptr;
    a.hist_items = hist_items;
    a.hist_weights = hist_weights;
    a.users = users;
    a.scores = scores;
    a.idx_stride = idx_stride;
    a.row_stride = row_stride;
    a.user_num = user_num;
    a.n = (int)n;
    a.n_items = (int)n_items;
    a.m = m;
    a.item_tiles = (int)((n_items + KNN_T - 1) / KNN_T);
    const int64_t grid = (int64_t)a.item_tiles * n;
    PMGT_CHECK(grid <= 0x7FFFFFFF, -2, "pmgt_knn_score: %lld workgroups exceed the grid limit; split the users", (long long)grid);
    hipStream_t st = (hipStream_t)stream;
    if (hist_weights) hipLaunchKernelGGL(knn_score_kernel<true>, dim3((unsigned)grid), dim3(KNN_THREADS), 0, st, a);
    else hipLaunchKernelGGL(knn_score_kernel<false>, dim3((unsigned)grid), dim3(KNN_THREADS), 0, st, a);
    PMGT_LAUNCH_OK();
    return 0;
}
