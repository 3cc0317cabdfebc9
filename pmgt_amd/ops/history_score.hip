// Item-kNN scoring of users from their histories (pmgt_history_score of include/pmgt_capi.h): score(u, j) = agg over i in H(u) of s(i, j), with
// s the item-by-item score of item_sim.hip (dot or cosine of two rows of ONE table) and H(u) the user's row of a CSR over user ids.  It is
// item_sim.hip's 128 x 128 tile with a segmented reduction over the query rows in its epilogue: the [sum |H(u)|, I] block of item scores
// never reaches memory, the output is [n, I].  Kept out of csrc/ for ncf_score.hip's reason: the measured step launches nothing of this.
//
// THE SCORE.  s(i, j) has the bits of pmgt_item_sim_score: dot = the fp32 fmaf chain over k ascending from 0 on v_mfma_f32_32x32x2_f32,
// cosine = (dot * inv[min(i, j)]) * inv[max(i, j)].  With i_0, i_1, .. the items of the user's list IN THE ORDER OF THE LIST (ascending ids,
// no duplicates: the caller builds it so):
//   max:   the largest s(i_t, j); NaN if any term is NaN; a zero result is +0.0
//   mean:  acc = s(i_0, j); acc = acc + s(i_t, j) for t = 1 .. len - 1, every sum rounded to fp32, none contracted; acc / float(len), one
//          IEEE division
// A workgroup owns WHOLE users and one thread owns a (user, candidate) pair from the first row of the user to the last, whatever the number
// of 128-row chunks the list spans: the order of the sums is the order of the list and nothing else, so the bits of score(u, j) depend on
// H(u), the rows of its items and row j alone -- not on n, the user's slot, the other users of the call or how the catalogue is cut.
//
// TILE.  A workgroup of 4 waves owns HS_G = 48 consecutive batch slots and 128 candidates.  The lists of its users, one after the other,
// are a sequence of T rows; it walks them in chunks of 128 (the last chunk of a group is partly empty: half a chunk on average, which 48
// users dilute better than 16).  Row m of a chunk is gathered from the table through the item id (rid[m], the
// way item_sim.hip gathers through qid), the k-loop is item_sim_score_kernel's at 2 x 2 waves of 2 x 2 blocks (32-column chunks of both
// operands through LDS at stride 33, the next chunk's global loads under the MFMAs).  The scaled 128 x 128 block is then STAGED in LDS
// at stride 129 (it aliases the operand buffers: a barrier after the last k-step, one after the staging, and the k-loop's own first
// barrier before the next chunk's operands).  Staging writes 32 consecutive floats per 32-lane half and the walk below reads 32
// consecutive floats per half: ds_write_b32 / ds_read_b32 bank by (address / 4) mod 32 within a half, so both are conflict-free at any
// stride.  Thread t walks candidate column t & 127 for the slots 24 (t >> 7) .. 24 (t >> 7) + 23 (their rows are one contiguous range of the
// sequence; all 64 lanes of a wave walk the same rows, so the loop is uniform): it reads eight rows at once, folds the rows of the open
// user in order, and when the sequence passes the end of a list it stores that user's score.  66 KiB of LDS: 2 workgroups a CU.
// With d a multiple of 4 and an aligned table (16-byte loads) the kernel takes 209 VGPRs; else (single-float loads) 256 and 16 AGPRs, one
// workgroup a CU.
// A slot past n is not stored.  A user id outside [0, user_num) or an empty list is never dereferenced: its row of scores is NaN.  An item
// id outside [0, n_items) in a list is never dereferenced either: its terms are NaN.  Output offsets are 64-bit.  No atomics anywhere.
#include "ncf_head.h"

namespace pmgt {

static constexpr int HS_THREADS = 256, HS_CHUNK = 32, HS_STRIDE = HS_CHUNK + 1, HS_T = 128, HS_STAGE = HS_T + 1, HS_G = 48;
static constexpr int HS_SEARCH = 32;                        // the first step of the slot search: a power of two, 2 HS_SEARCH >= HS_G
static_assert(HS_G % 2 == 0 && HS_G >= 2 && HS_G <= 2 * HS_SEARCH && HS_G <= HS_T, "the slots of a group");

struct HistArgs {
    const float* table;        // [n_items][d]
    const float* inv;          // [n_items] or NULL (metric "dot")
    const int64_t* hist_ptr;   // [user_num + 1]
    const int32_t* hist_items;
    const int64_t* users;      // [n]
    float* scores;             // [n][row_stride]
    int64_t row_stride, user_num;
    int n, n_items, d, item_tiles;
};

// item_sim.hip's operand fetch at 128 rows: rows x k-columns [k0, k0 + 32), zero past the live rows and past d: global -> registers
// ids == NULL: the rows are the table's own (candidates); else they are gathered through the LDS copy of the chunk's item ids (< 0: none)
template <bool VEC> __device__ __forceinline__ void hist_fetch(float (&st)[HS_T / 8], const float* __restrict__ table, const int* ids, int64_t row0,
                                                                int live, int d, int k0, int tid) {
    if constexpr (VEC) {
#pragma unroll
        for (int i = 0; i < HS_T / 32; ++i) {
            const int e = tid + HS_THREADS * i, c = (e & 7) * 4, m = e >> 3;
            int64_t row = -1;
            if (ids) row = ids[m];
            else if (row0 + m < live) row = row0 + m;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row >= 0 && k0 + c < d) v = *reinterpret_cast<const float4*>(table + row * d + k0 + c);
            st[4 * i] = v.x, st[4 * i + 1] = v.y, st[4 * i + 2] = v.z, st[4 * i + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < HS_T / 8; ++i) {
            const int e = tid + HS_THREADS * i, c = e & 31, m = e >> 5;
            int64_t row = -1;
            if (ids) row = ids[m];
            else if (row0 + m < live) row = row0 + m;
            st[i] = (row >= 0 && k0 + c < d) ? table[row * d + k0 + c] : 0.f;
        }
    }
}
template <bool VEC> __device__ __forceinline__ void hist_store(const float (&st)[HS_T / 8], float* ws, int tid) {
    if constexpr (VEC) {
#pragma unroll
        for (int i = 0; i < HS_T / 32; ++i) {
            const int e = tid + HS_THREADS * i, c = (e & 7) * 4, m = e >> 3;
#pragma unroll
            for (int t = 0; t < 4; ++t) ws[m * HS_STRIDE + c + t] = st[4 * i + t];
        }
    } else {
#pragma unroll
        for (int i = 0; i < HS_T / 8; ++i) {
            const int e = tid + HS_THREADS * i, c = e & 31, m = e >> 5;
            ws[m * HS_STRIDE + c] = st[i];
        }
    }
}

template <bool VEC, bool MEAN> __global__ __launch_bounds__(HS_THREADS) void history_score_kernel(HistArgs a) {
    __shared__ float buf[HS_T * HS_STAGE];                   // the operands of a k-chunk, then the staged block (aliased)
    __shared__ int rid[HS_T];                                // the chunk's item ids; -1 = past the sequence, -2 = an id outside the table (its terms are NaN)
    __shared__ float rinv[HS_T];                             // their inverse norms (cosine)
    __shared__ int64_t s_off[HS_G + 1];                      // where each slot's list begins in the group's sequence of rows
    __shared__ int64_t s_start[HS_G];                        // ... and in hist_items
    float* const qs = buf;
    float* const cs = buf + HS_T * HS_STRIDE;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, p = lane & 31, h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const int64_t j0 = (int64_t)(blockIdx.x % (unsigned)a.item_tiles) * HS_T;
    const int r0 = (int)(blockIdx.x / (unsigned)a.item_tiles) * HS_G;
    const int d = a.d;
    if (tid < 64) {                                          // wave 0: the slots' lists (where they begin in hist_items, how long they are) and
        int64_t start = 0, len = 0;                          // the exclusive prefix of their lengths, by a shuffle scan
        if (tid < HS_G && r0 + tid < a.n) {
            const int64_t u = a.users[r0 + tid];
            if (u >= 0 && u < a.user_num) {
                start = a.hist_ptr[u];
                len = a.hist_ptr[u + 1] - start;
                if (len < 0) len = 0;
            }
        }
        int64_t upto = len;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int64_t below = __shfl_up(upto, o);
            if (tid >= o) upto += below;
        }
        if (tid < HS_G) s_start[tid] = start, s_off[tid] = upto - len;
        if (tid == HS_G - 1) s_off[HS_G] = upto;
    }
    __syncthreads();
    const int64_t total = s_off[HS_G];
    const bool cosine = a.inv != nullptr;
    // the walk's state: this thread folds column `col` for the slots [cur, last) in order; `next` = where the open slot's list ends
    const int col = tid & (HS_T - 1), first_slot = (tid >> 7) * (HS_G / 2), last_slot = first_slot + HS_G / 2;
    const int64_t jcol = j0 + col, walk_lo = s_off[first_slot], walk_hi = s_off[last_slot];
    int cur = first_slot;
    int64_t next = s_off[cur + 1];
    float acc = 0.f;
    bool open = false, bad = false;
    auto flush = [&]() {                                     // the open slot is complete: store its score, open the next one
        const int r = r0 + cur;
        if (r < a.n && jcol < a.n_items) {
            const int64_t len = next - s_off[cur];
            float v;
            if (len <= 0) v = __builtin_nanf("");
            else if constexpr (MEAN) v = __fdiv_rn(acc, (float)len);
            else v = bad ? __builtin_nanf("") : (acc == 0.f ? 0.f : acc);
            a.scores[(int64_t)r * a.row_stride + jcol] = v;
        }
        ++cur;
        next = s_off[min(cur + 1, HS_G)];
        acc = 0.f, open = false, bad = false;
    };
    const float* qw = qs + (wm * 64 + p) * HS_STRIDE + h;
    const float* cw = cs + (wn * 64 + p) * HS_STRIDE + h;
    for (int64_t c0 = 0; c0 < total; c0 += HS_T) {
        if (tid < HS_T) {                                    // (the previous chunk's epilogue is behind the barrier after its staging)
            const int64_t idx = c0 + tid;
            int id = -1;
            if (idx < total) {
                int s = 0;
#pragma unroll
                for (int step = HS_SEARCH; step >= 1; step >>= 1)      // the LAST slot that begins at or before idx: the one that holds it
                    if (s + step < HS_G && s_off[s + step] <= idx) s += step;
                const int it = a.hist_items[s_start[s] + (idx - s_off[s])];
                id = (it >= 0 && it < a.n_items) ? it : -2;
            }
            rid[tid] = id;
            rinv[tid] = (id >= 0 && cosine) ? a.inv[id] : 0.f;
        }
        __syncthreads();
        f32x16 blk[2][2];
#pragma unroll
        for (int bm = 0; bm < 2; ++bm)
#pragma unroll
            for (int bn = 0; bn < 2; ++bn)
#pragma unroll
                for (int g = 0; g < 16; ++g) blk[bm][bn][g] = 0.f;
        float sq[HS_T / 8], sc[HS_T / 8];
        hist_fetch<VEC>(sq, a.table, rid, 0, 0, d, 0, tid);
        hist_fetch<VEC>(sc, a.table, nullptr, j0, a.n_items, d, 0, tid);
        for (int k0 = 0; k0 < d; k0 += HS_CHUNK) {
            __syncthreads();                                 // every wave is done with the previous k-chunk, and with the previous staged block
            hist_store<VEC>(sq, qs, tid);
            hist_store<VEC>(sc, cs, tid);
            __syncthreads();
            if (k0 + HS_CHUNK < d) {
                hist_fetch<VEC>(sq, a.table, rid, 0, 0, d, k0 + HS_CHUNK, tid);
                hist_fetch<VEC>(sc, a.table, nullptr, j0, a.n_items, d, k0 + HS_CHUNK, tid);
            }
            const int kc = min(HS_CHUNK, d - k0);
            for (int s0 = 0; s0 < kc; s0 += 8)               // (uniform; the k-steps past d multiply zeros)
#pragma unroll
                for (int s = s0; s < s0 + 8; s += 2) {
                    float qa[2], cb[2];
#pragma unroll
                    for (int bm = 0; bm < 2; ++bm) qa[bm] = qw[bm * 32 * HS_STRIDE + s];
#pragma unroll
                    for (int bn = 0; bn < 2; ++bn) cb[bn] = cw[bn * 32 * HS_STRIDE + s];
#pragma unroll
                    for (int bm = 0; bm < 2; ++bm)
#pragma unroll
                        for (int bn = 0; bn < 2; ++bn) blk[bm][bn] = __builtin_amdgcn_mfma_f32_32x32x2f32(qa[bm], cb[bn], blk[bm][bn], 0, 0, 0);
                }
        }
        __syncthreads();                                     // the last k-step has read its operands: the staged block may overwrite them
        // register g of block (bm, bn) = chunk row 32 (2 wm + bm) + rho(g) + 4 h, candidate j0 + 32 (2 wn + bn) + p: scale, then stage
#pragma unroll
        for (int bn = 0; bn < 2; ++bn) {
            const int c = (wn * 2 + bn) * 32 + p;
            const int64_t j = j0 + c;
            const float inv_j = (cosine && j < a.n_items) ? a.inv[j] : 1.f;
#pragma unroll
            for (int bm = 0; bm < 2; ++bm)
#pragma unroll
                for (int g = 0; g < 16; ++g) {
                    const int m = (wm * 2 + bm) * 32 + rho(g) + 4 * h;
                    const int i = rid[m];
                    float s = blk[bm][bn][g];
                    if (i == -2) {
                        s = __builtin_nanf("");
                    } else if (cosine) {
                        const float inv_i = rinv[m];
                        s = i <= j ? (s * inv_i) * inv_j : (s * inv_j) * inv_i;
                    }
                    buf[m * HS_STAGE + c] = s;
                }
        }
        __syncthreads();
        // the walk: rows [lo, hi) of the chunk are its share of this thread's slots.  Eight rows are read at once (the reads of a row do
        // not wait for the fold of the row before), then folded one after the other, in order
        auto in_chunk = [&](int64_t at) { return (int)min(max(at - c0, (int64_t)0), (int64_t)HS_T); };      // a place of the sequence, clamped to the chunk
        const int lo = in_chunk(walk_lo), hi = in_chunk(min(total, walk_hi));
        int end = in_chunk(next);                            // where the open slot's list ends (HS_T: not in this chunk)
        for (int m0 = lo; m0 < hi; m0 += 8) {
            float v[8];
#pragma unroll
            for (int t = 0; t < 8; ++t) v[t] = buf[min(m0 + t, HS_T - 1) * HS_STAGE + col];      // (past hi: read, not used)
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                if (m0 + t >= hi) break;
                while (m0 + t >= end) {
                    flush();
                    end = in_chunk(next);
                }
                if constexpr (MEAN) {
                    acc = open ? __fadd_rn(acc, v[t]) : v[t];
                } else {
                    bad = bad || v[t] != v[t];
                    acc = (!open || v[t] > acc) ? v[t] : acc;
                }
                open = true;
            }
        }
    }
    while (cur < last_slot) flush();                         // the slots whose lists have ended, the empty ones among them
}

template <bool VEC, bool MEAN> static int hist_launch(HistArgs& a, hipStream_t st) {
    a.item_tiles = (int)(((int64_t)a.n_items + HS_T - 1) / HS_T);
    const int64_t grid = (int64_t)a.item_tiles * ((a.n + HS_G - 1) / HS_G);
    PMGT_CHECK(grid <= 0x7FFFFFFF, -2, "pmgt_history_score: %lld workgroups exceed the grid limit; split the users", (long long)grid);
    hipLaunchKernelGGL((history_score_kernel<VEC, MEAN>), dim3((unsigned)grid), dim3(HS_THREADS), 0, st, a);
    return 0;
}

}  // namespace pmgt

using namespace pmgt;

extern "C" int pmgt_history_score(const float* table, const float* inv_norm, const int64_t* hist_ptr, const int32_t* hist_items,
                                  const int64_t* users, int64_t n, int64_t user_num, int64_t n_items, int d, int agg, float* scores,
                                  int64_t row_stride, void* stream) {
    PMGT_CHECK(d >= 1 && d <= PMGT_ITEM_SIM_MAX_D, -2, "pmgt_history_score: d = %d outside [1, %d]", d, PMGT_ITEM_SIM_MAX_D);
    PMGT_CHECK(n >= 1 && n <= PMGT_NCF_MAX_USERS, -2, "pmgt_history_score: n = %lld users outside [1, %d]", (long long)n, PMGT_NCF_MAX_USERS);
    PMGT_CHECK(n_items >= 1 && n_items <= 0x7FFFFFFELL, -2, "pmgt_history_score: %lld items outside [1, 2^31 - 2]", (long long)n_items);
    PMGT_CHECK(user_num >= 1, -2, "pmgt_history_score: user_num = %lld below 1", (long long)user_num);
    PMGT_CHECK(row_stride >= n_items, -2, "pmgt_history_score: row_stride = %lld below the %lld items", (long long)row_stride, (long long)n_items);
    PMGT_CHECK(agg == PMGT_HISTORY_MEAN || agg == PMGT_HISTORY_MAX, -2, "pmgt_history_score: unknown agg %d", agg);
    PMGT_CHECK(table && hist_ptr && hist_items && users && scores, -2, "pmgt_history_score: NULL buffer");
    PMGT_CHECK((((uintptr_t)table | (uintptr_t)inv_norm | (uintptr_t)scores | (uintptr_t)hist_items) & 3) == 0
                   && (((uintptr_t)users | (uintptr_t)hist_ptr) & 7) == 0,
               -2, "pmgt_history_score: misaligned buffer");
    HistArgs a;
    a.table = table;
    a.inv = inv_norm;
    a.hist_ptr = hist_ptr;
    a.hist_items = hist_items;
    a.users = users;
    a.scores = scores;
    a.row_stride = row_stride;
    a.user_num = user_num;
    a.n = (int)n;
    a.n_items = (int)n_items;
    a.d = d;
    a.item_tiles = 0;
    hipStream_t st = (hipStream_t)stream;
    const bool vec = (d & 3) == 0 && ((uintptr_t)table & 15) == 0;      // every row then starts on 16 bytes
    const bool mean = agg == PMGT_HISTORY_MEAN;
    const int rc = vec ? (mean ? hist_launch<true, true>(a, st) : hist_launch<true, false>(a, st))
                       : (mean ? hist_launch<false, true>(a, st) : hist_launch<false, false>(a, st));
    if (rc) return rc;
    PMGT_LAUNCH_OK();
    return 0;
}
