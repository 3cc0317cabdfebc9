// The item graph from interactions (pmgt_item_graph_count, pmgt_item_graph_fill of include/pmgt_capi.h): the reference's "Construct Product
// Graph" cell (notebooks/PMGT.ipynb, cell 20) without the matrix product.  With A the binary item-by-user matrix, C = A A^T counts the
// users two items share; an edge is an off-diagonal entry with C[i][j] >= min_count.  Kept out of csrc/ for eval_metrics.hip's reason: the
// measured step launches nothing of this.
//
// INPUT: the two CSR images of the deduplicated pairs, item -> users (any order inside a row) and user -> items.  Row i of C is the
// expansion  { j : u in users(i), j in items(u), j != i }  with multiplicity; `work[i]` is its length (the caller's segment sum).
//
// TWO PASSES over the same expansion, both integer only:
//   count   the multiplicities of a row are accumulated in an LDS hash table (open addressing, linear probing, a power of two of slots,
//           integer atomics); deg[i] = the slots that reach min_count; the largest count seen anywhere goes to one word by atomicMax
//   fill    after the caller's exclusive scan of deg: the same expansion, the qualifying (j, count) are compacted to the front of the table,
//           sorted by j ascending with a bitonic network in LDS (as topk_rows.hip sorts its survivors) and stored at the row's offset, j as
//           its node id.  Both directions of an edge are produced by their own rows: no transpose pass, no second sort.  An
//           upper-triangle-only variant would halve the inserts but need a sort of the whole edge list by destination afterwards; it is
//           not built and was not measured.
// Counts are sums and the stored order comes from the sort, never from the order in which atomics land or slots are taken: two calls on
// the same inputs give the same bits.
//
// SCHEDULING, one policy for all rows, decided in the kernel from work[i]: a 256-thread workgroup takes four consecutive rows.
//   phase A  every wave takes its own row if work <= 3/4 slots: a table of `slots` entries of the wave's own.  Such a row cannot overflow.
//   phase B  the longer rows are taken one after the other by the whole workgroup with the four tables joined (4 slots entries).
//   Inside a row the lanes take one user each and walk that user's items; a user with more than 64 items is walked by the whole wave.
// A table is filled to 3/4 at most (linear probing stays short): the distinct keys are counted as their slots are claimed.
// A ROW THAT DOES NOT FIT (more than 3 slots distinct neighbours) does not spin and is not dropped: the claim beyond the limit raises the
// row's flag, every lane leaves at its next insert, and a probe sequence ends after one trip round the table whatever happens.  The flag
// (bit 31 of deg_flags[i]) is a function of the row -- its number of distinct neighbours -- not of timing.  The row is redone by the
// DENSE FALLBACK: one uint32 [num_item] scratch row per workgroup from a bounded pool, global
// integer atomics, then one ascending scan of the row that counts or stores the qualifying entries and clears what it finds.  The
// scratch is zero before and after every call.
#include "../../include/pmgt_capi.h"
#include "../csrc/common.h"

namespace pmgt {

static constexpr int IG_THREADS = 256, IG_WAVES = IG_THREADS / 64, IG_ROWS = IG_WAVES;      // rows a workgroup takes
static constexpr uint32_t IG_EMPTY = 0xFFFFFFFFu;            // no item has this index (num_item <= 2^31 - 2)
static constexpr int IG_LONG_USER = 64;                      // a user with more items is walked by the whole wave
static constexpr int IG_DENSE_PER_THREAD = 16, IG_DENSE_CHUNK = IG_THREADS * IG_DENSE_PER_THREAD;      // entries of the scratch row a scan step covers
static constexpr int64_t IG_MAX_ITEMS = 0x7FFFFFFELL;

struct ItemGraphArgs {
    const int64_t* item_ptr;     // [num_item + 1]
    const int32_t* item_users;   // [n_pairs] compact user index
    const int64_t* user_ptr;     // [n_users + 1]
    const int32_t* user_items;   // [n_pairs]
    const int64_t* work;         // [num_item]
    uint32_t* deg_flags;         // [num_item]: count writes deg | flag << 31, fill reads it
    uint32_t* max_count;         // count: one word
    const int64_t* row_ptr;      // fill: [num_item + 1]
    const int32_t* node_of_item; // fill: [num_item]
    int32_t* indices;            // fill: [total]
    int32_t* counts;             // fill: [total]
    uint32_t* scratch;           // [scratch_rows][scratch_stride], zero
    int64_t scratch_rows, scratch_stride;
    int64_t num_item, n_users, n_pairs, total;
    uint32_t min_count;
    int slots, log_slots;
};

__device__ __forceinline__ int64_t ig_clamp(int64_t v, int64_t hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

// A table holds at most `limit` = 3/4 of its slots distinct keys: the claim that goes beyond raises *flag, and every later insert returns
// at once.  Probing ends after one trip round the table at the latest (with the limit below the size it finds an empty slot long before).
__device__ __forceinline__ void ig_insert(uint32_t* keys, uint32_t* cnt, uint32_t mask, int log_n, int limit, int* n_keys, int* flag, uint32_t j) {
    if (__hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return;
    uint32_t s = (j * 2654435761u) >> (32 - log_n);
    for (uint32_t p = 0; p <= mask; ++p) {
        uint32_t k = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (k == IG_EMPTY) {
            const uint32_t old = atomicCAS(&keys[s], IG_EMPTY, j);
            k = old;
            if (old == IG_EMPTY) {
                k = j;
                if (atomicAdd(n_keys, 1) + 1 > limit) break;      // one key too many: the row is the fallback's
            }
        }
        if (k == j) {
            atomicAdd(&cnt[s], 1u);
            return;
        }
        s = (s + 1u) & mask;
    }
    __hip_atomic_store(flag, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the expansion of `row` by n_waves waves (this one is wave `w` of them); ins(j) for every (user of row, item j != row of that user);
// stops early once *stop is set.  Every lane of the wave runs the same trips.
template <class Insert>
__device__ __forceinline__ void ig_expand(const ItemGraphArgs& a, int64_t row, int w, int n_waves, int lane, const int* stop, Insert&& ins) {
    const int64_t lo = ig_clamp(a.item_ptr[row], a.n_pairs), hi = ig_clamp(a.item_ptr[row + 1], a.n_pairs);
    for (int64_t e0 = lo + (int64_t)w * 64; e0 < hi; e0 += (int64_t)n_waves * 64) {
        const int stopped = __hip_atomic_load(stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (__builtin_amdgcn_ballot_w64(stopped != 0)) break;      // (uniform)
        const int64_t e = e0 + lane;
        long long ulo = 0, uhi = 0;
        if (e < hi) {
            const int64_t u = a.item_users[e];
            if (u >= 0 && u < a.n_users) {
                ulo = ig_clamp(a.user_ptr[u], a.n_pairs);
                uhi = ig_clamp(a.user_ptr[u + 1], a.n_pairs);
            }
        }
        const bool long_user = uhi - ulo > IG_LONG_USER;
        if (!long_user)
            for (long long k = ulo; k < uhi; ++k) {
                const int64_t j = a.user_items[k];
                if (j != row && j >= 0 && j < a.num_item) ins((uint32_t)j);
            }
        unsigned long long m = __builtin_amdgcn_ballot_w64(long_user);
        while (m) {                                              // (uniform)
            if (__builtin_amdgcn_ballot_w64(__hip_atomic_load(stop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) != 0)) break;
            const int src = __builtin_ctzll(m);
            m &= m - 1ull;
            const long long l = __shfl(ulo, src, 64), h = __shfl(uhi, src, 64);
            for (long long k = l + lane; k < h; k += 64) {
                const int64_t j = a.user_items[k];
                if (j != row && j >= 0 && j < a.num_item) ins((uint32_t)j);
            }
        }
    }
}

// FILL = false: the count pass; FILL = true: the fill pass.  LDS: keys uint32 [4 slots], cnt uint32 [4 slots] (dynamic).
template <bool FILL>
__global__ __launch_bounds__(IG_THREADS) void item_graph_rows_kernel(ItemGraphArgs a) {
    extern __shared__ uint32_t ig_lds[];
    __shared__ int ovf[IG_ROWS], n_keys[IG_ROWS];
    __shared__ uint32_t wq[IG_WAVES], wm[IG_WAVES];
    const int S = a.slots, L = a.log_slots, NS = S * IG_WAVES, SW = S / 4 * 3;      // SW: the expansion a wave's table surely holds
    uint32_t* keys = ig_lds;
    uint32_t* cnt = ig_lds + NS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * IG_ROWS;
    // 0: nothing to do, 1: the wave's own row (phase A), 2: the workgroup's (phase B); uniform per row
    int mode[IG_ROWS];
#pragma unroll
    for (int r = 0; r < IG_ROWS; ++r) {
        const int64_t row = r0 + r;
        mode[r] = 0;
        if (row < a.num_item) {
            const int64_t wk = a.work[row];
            if (FILL) {
                const uint32_t df = a.deg_flags[row];
                mode[r] = (df & 0x80000000u) || (df & 0x7FFFFFFFu) == 0u ? 0 : (wk <= SW ? 1 : 2);      // flagged: the fallback's; no edge: nothing to store
            } else {
                mode[r] = wk <= 0 ? 0 : (wk <= SW ? 1 : 2);
            }
        }
    }
    if (tid < IG_ROWS) { ovf[tid] = 0; n_keys[tid] = 0; }
    uint32_t seen_max = 0u;
    // phase A and the four rounds of phase B share one body: `round` -1 is phase A
    for (int round = -1; round < IG_ROWS; ++round) {             // (uniform)
        const bool phase_a = round < 0;
        bool any = false;
#pragma unroll
        for (int r = 0; r < IG_ROWS; ++r) any |= phase_a ? mode[r] == 1 : (r == round && mode[r] == 2);
        if (!any) continue;                                      // (uniform)
        const int my = phase_a ? wave : round;                   // the row of this thread's group
        bool active = false;
#pragma unroll
        for (int r = 0; r < IG_ROWS; ++r) active |= r == my && mode[r] == (phase_a ? 1 : 2);
        const int64_t row = r0 + my;
        const int G = phase_a ? 64 : IG_THREADS, gt = phase_a ? lane : tid;      // the group's size, this thread's place in it
        const int base = phase_a ? wave * S : 0, n = phase_a ? S : NS, ln = phase_a ? L : L + 2;
        for (int t = tid; t < NS; t += IG_THREADS) { keys[t] = IG_EMPTY; cnt[t] = 0u; }
        __syncthreads();
        if (active) {
            uint32_t* kk = keys + base;
            uint32_t* cc = cnt + base;
            const uint32_t mask = (uint32_t)n - 1u;
            int* flag = &ovf[my];
            int* nk = &n_keys[my];
            const int limit = n / 4 * 3;
            ig_expand(a, row, phase_a ? 0 : wave, phase_a ? 1 : IG_WAVES, lane, flag, [&](uint32_t j) { ig_insert(kk, cc, mask, ln, limit, nk, flag, j); });
        }
        __syncthreads();
        const bool full = active && ovf[my] != 0;                // (a phase A row cannot be: work <= 3/4 slots)
        if (!FILL) {
            uint32_t q = 0u, mx = 0u;
            if (active && !full)
                for (int t = gt; t < n; t += G) {
                    const uint32_t v = cnt[base + t];
                    q += v >= a.min_count ? 1u : 0u;
                    mx = v > mx ? v : mx;
                }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                q += __shfl_xor(q, o, 64);
                const uint32_t other = __shfl_xor(mx, o, 64);
                mx = other > mx ? other : mx;
            }
            seen_max = mx > seen_max ? mx : seen_max;
            if (lane == 0) wq[wave] = q;
            __syncthreads();
            if (active && gt == 0) {
                const uint32_t deg = phase_a ? wq[wave] : ((wq[0] + wq[1]) + wq[2]) + wq[3];
                a.deg_flags[row] = full ? 0x80000000u : deg;
            }
            __syncthreads();
            continue;
        }
        // ---- fill: compact the qualifying slots to the front of the group's table, in place: chunk c of the table is read whole before
        //      anything of it is written, and what is written lies below the next chunk
        int m = 0;
        for (int c0 = 0; c0 < n; c0 += G) {                      // (uniform: n / G = slots / 64 in both phases; below 64 slots one short chunk)
            uint32_t k = IG_EMPTY, v = 0u;
            if (active && !full && c0 + gt < n) { k = keys[base + c0 + gt]; v = cnt[base + c0 + gt]; }
            const bool q = v >= a.min_count;
            const unsigned long long b = __builtin_amdgcn_ballot_w64(q);
            const int pre = __builtin_popcountll(b & ((1ull << lane) - 1ull));
            if (lane == 0) wq[wave] = (uint32_t)__builtin_popcountll(b);
            __syncthreads();
            int off = 0, tot = (int)wq[wave];
            if (!phase_a) {
                tot = 0;
                for (int w = 0; w < IG_WAVES; ++w) {
                    off += w < wave ? (int)wq[w] : 0;
                    tot += (int)wq[w];
                }
            }
            if (q) { keys[base + m + off + pre] = k; cnt[base + m + off + pre] = v; }
            m += tot;
            __syncthreads();
        }
        // ---- sort the m entries by item, ascending: pad to a power of two P (the same for the four groups of phase A)
        if (lane == 0) wm[wave] = (uint32_t)m;
        __syncthreads();
        int mmax = m;
        if (phase_a) mmax = max(max((int)wm[0], (int)wm[1]), max((int)wm[2], (int)wm[3]));
        int P = 1;
        while (P < mmax) P <<= 1;
        for (int t = m + gt; t < P; t += G) { keys[base + t] = IG_EMPTY; cnt[base + t] = 0u; }
        __syncthreads();
        for (int size = 2; size <= P; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int t = gt; t < (P >> 1); t += G) {
                    const int lo = ((t / stride) * stride << 1) + (t % stride), hi = lo + stride;
                    const bool asc = (lo & size) == 0;
                    const uint32_t u = keys[base + lo], v = keys[base + hi];
                    if ((u > v) == asc) {
                        const uint32_t cu = cnt[base + lo], cv = cnt[base + hi];
                        keys[base + lo] = v; keys[base + hi] = u;
                        cnt[base + lo] = cv; cnt[base + hi] = cu;
                    }
                }
                __syncthreads();
            }
        if (active && !full) {
            const int64_t at = a.row_ptr[row], room = a.row_ptr[row + 1] - at;
            for (int t = gt; t < m; t += G) {
                const uint32_t j = keys[base + t];
                if (t < room && at + t >= 0 && at + t < a.total && j < (uint32_t)a.num_item) {
                    a.indices[at + t] = a.node_of_item[j];
                    a.counts[at + t] = (int32_t)cnt[base + t];
                }
            }
        }
        __syncthreads();
    }
    if (!FILL) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t other = __shfl_xor(seen_max, o, 64);
            seen_max = other > seen_max ? other : seen_max;
        }
        if (lane == 0 && seen_max > 0u) atomicMax(a.max_count, seen_max);      // integer max: no order in it
    }
}

// the dense fallback: workgroup b owns scratch row b and redoes the flagged rows b, b + pool, b + 2 pool, ...
template <bool FILL>
__global__ __launch_bounds__(IG_THREADS) void item_graph_dense_kernel(ItemGraphArgs a) {
    __shared__ int64_t todo[IG_THREADS];
    __shared__ int n_todo, never;
    __shared__ uint32_t wtot[IG_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t pool = gridDim.x;
    uint32_t* srow = a.scratch + (int64_t)blockIdx.x * a.scratch_stride;
    if (tid == 0) never = 0;
    uint32_t seen_max = 0u;
    for (int64_t b0 = 0; blockIdx.x + pool * b0 < a.num_item; b0 += IG_THREADS) {      // (uniform)
        if (tid == 0) n_todo = 0;
        __syncthreads();
        const int64_t cand = blockIdx.x + pool * (b0 + tid);
        if (cand < a.num_item && (a.deg_flags[cand] & 0x80000000u)) todo[atomicAdd(&n_todo, 1)] = cand;      // (the order of the rows does not matter)
        __syncthreads();
        const int nt = n_todo;
        for (int i = 0; i < nt; ++i) {                           // (uniform)
            const int64_t row = todo[i];
            ig_expand(a, row, wave, IG_WAVES, lane, &never, [&](uint32_t j) { atomicAdd(&srow[j], 1u); });
            __threadfence();
            __syncthreads();
            __threadfence();                                     // the scan below reads what the atomics left in L2, not an older line
            const int64_t at = FILL ? a.row_ptr[row] : 0, room = FILL ? a.row_ptr[row + 1] - at : 0;
            int64_t done = 0;
            uint32_t q_mine = 0u;
            for (int64_t c0 = 0; c0 < a.num_item; c0 += IG_DENSE_CHUNK) {      // (uniform)
                const int64_t j0 = c0 + (int64_t)tid * IG_DENSE_PER_THREAD;
                uint32_t v[IG_DENSE_PER_THREAD];
                uint32_t q = 0u;
#pragma unroll
                for (int g = 0; g < IG_DENSE_PER_THREAD; g += 4) {
                    uint4 x = make_uint4(0u, 0u, 0u, 0u);
                    if (j0 + g < a.scratch_stride) {             // (the stride is a multiple of 4: a vector is inside the row or outside it)
                        x = *(const uint4*)(srow + j0 + g);
                        if (x.x | x.y | x.z | x.w) *(uint4*)(srow + j0 + g) = make_uint4(0u, 0u, 0u, 0u);
                    }
                    v[g] = x.x; v[g + 1] = x.y; v[g + 2] = x.z; v[g + 3] = x.w;
                }
#pragma unroll
                for (int g = 0; g < IG_DENSE_PER_THREAD; ++g) {
                    q += v[g] >= a.min_count ? 1u : 0u;
                    seen_max = v[g] > seen_max ? v[g] : seen_max;
                }
                if (!FILL) {
                    q_mine += q;
                    continue;
                }
                // exclusive scan of q over the workgroup: ascending threads hold ascending items
                uint32_t incl = q;
#pragma unroll
                for (int o = 1; o < 64; o <<= 1) {
                    const uint32_t up = __shfl_up(incl, o, 64);
                    if (lane >= o) incl += up;
                }
                if (lane == 63) wtot[wave] = incl;
                __syncthreads();
                uint32_t pos = incl - q, tot = 0u;
                for (int w = 0; w < IG_WAVES; ++w) {
                    pos += w < wave ? wtot[w] : 0u;
                    tot += wtot[w];
                }
                int64_t k = done + pos;
#pragma unroll
                for (int g = 0; g < IG_DENSE_PER_THREAD; ++g)
                    if (v[g] >= a.min_count) {
                        const int64_t j = j0 + g;
                        if (k < room && at + k >= 0 && at + k < a.total && j < a.num_item) {
                            a.indices[at + k] = a.node_of_item[j];
                            a.counts[at + k] = (int32_t)v[g];
                        }
                        ++k;
                    }
                done += tot;
                __syncthreads();
            }
            if (!FILL) {
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) q_mine += __shfl_xor(q_mine, o, 64);
                if (lane == 0) wtot[wave] = q_mine;
                __syncthreads();
                if (tid == 0) a.deg_flags[row] = 0x80000000u | (((wtot[0] + wtot[1]) + wtot[2]) + wtot[3]);
            }
            __threadfence();                                     // the zeros are in L2 before the next row's atomics
            __syncthreads();
        }
    }
    if (!FILL) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const uint32_t other = __shfl_xor(seen_max, o, 64);
            seen_max = other > seen_max ? other : seen_max;
        }
        if (lane == 0 && seen_max > 0u) atomicMax(a.max_count, seen_max);
    }
}

static int ig_check(const char* who, const ItemGraphArgs& a, bool fill) {
    PMGT_CHECK(a.num_item >= 1 && a.num_item <= IG_MAX_ITEMS, -2, "%s: num_item = %lld outside [1, 2^31 - 2]", who, (long long)a.num_item);
    PMGT_CHECK(a.n_pairs >= 1 && a.n_pairs <= 0x7FFFFFFFLL, -2, "%s: n_pairs = %lld outside [1, 2^31 - 1]", who, (long long)a.n_pairs);
    PMGT_CHECK(a.n_users >= 1 && a.n_users <= a.n_pairs, -2, "%s: n_users = %lld outside [1, n_pairs]", who, (long long)a.n_users);
    PMGT_CHECK(a.min_count >= 1u && a.min_count <= 0x7FFFFFFFu, -2, "%s: min_count outside [1, 2^31 - 1]", who);
    PMGT_CHECK(a.slots >= PMGT_ITEM_GRAPH_MIN_SLOTS && a.slots <= PMGT_ITEM_GRAPH_MAX_SLOTS && (a.slots & (a.slots - 1)) == 0, -2,
               "%s: slots = %d is no power of two in [%d, %d]", who, a.slots, PMGT_ITEM_GRAPH_MIN_SLOTS, PMGT_ITEM_GRAPH_MAX_SLOTS);
    PMGT_CHECK(a.item_ptr && a.item_users && a.user_ptr && a.user_items && a.work && a.deg_flags && a.scratch, -2, "%s: NULL buffer", who);
    PMGT_CHECK(a.scratch_rows >= 1 && a.scratch_rows <= 65535, -2, "%s: scratch_rows = %lld outside [1, 65535]", who, (long long)a.scratch_rows);
    PMGT_CHECK((((uintptr_t)a.item_ptr | (uintptr_t)a.user_ptr | (uintptr_t)a.work | (uintptr_t)a.row_ptr) & 7) == 0 &&
               (((uintptr_t)a.item_users | (uintptr_t)a.user_items | (uintptr_t)a.deg_flags | (uintptr_t)a.max_count | (uintptr_t)a.node_of_item |
                 (uintptr_t)a.indices | (uintptr_t)a.counts) & 3) == 0 && ((uintptr_t)a.scratch & 15) == 0, -2, "%s: misaligned buffer", who);
    if (fill) {
        PMGT_CHECK(a.row_ptr && a.node_of_item && a.indices && a.counts, -2, "%s: NULL buffer", who);
        PMGT_CHECK(a.total >= 1, -2, "%s: total = %lld below 1", who, (long long)a.total);
    } else {
        PMGT_CHECK(a.max_count != nullptr, -2, "%s: NULL buffer", who);
    }
    return 0;
}

template <bool FILL>
static int ig_launch(ItemGraphArgs a, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    a.scratch_stride = (a.num_item + 3) / 4 * 4;
    a.log_slots = 0;
    while ((1 << a.log_slots) < a.slots) ++a.log_slots;
    const size_t lds = (size_t)a.slots * IG_WAVES * 2 * sizeof(uint32_t);      // <= 64 KiB
    const unsigned grid = (unsigned)((a.num_item + IG_ROWS - 1) / IG_ROWS);
    hipLaunchKernelGGL(item_graph_rows_kernel<FILL>, dim3(grid), dim3(IG_THREADS), lds, st, a);
    hipLaunchKernelGGL(item_graph_dense_kernel<FILL>, dim3((unsigned)a.scratch_rows), dim3(IG_THREADS), 0, st, a);
    PMGT_LAUNCH_OK();
    return 0;
}

}  // namespace pmgt

using namespace pmgt;

extern "C" {

int pmgt_item_graph_default_slots(void) { return PMGT_ITEM_GRAPH_DEFAULT_SLOTS; }

int pmgt_item_graph_count(const int64_t* item_ptr, const int32_t* item_users, const int64_t* user_ptr, const int32_t* user_items,
                          const int64_t* work, int64_t num_item, int64_t n_users, int64_t n_pairs, int64_t min_count, int slots,
                          uint32_t* deg_flags, uint32_t* max_count, uint32_t* scratch, int64_t scratch_rows, void* stream) {
    PMGT_CHECK(min_count >= 1 && min_count <= 0x7FFFFFFFLL, -2, "pmgt_item_graph_count: min_count = %lld outside [1, 2^31 - 1]", (long long)min_count);
    ItemGraphArgs a = {};
    a.item_ptr = item_ptr; a.item_users = item_users; a.user_ptr = user_ptr; a.user_items = user_items; a.work = work;
    a.deg_flags = deg_flags; a.max_count = max_count; a.scratch = scratch; a.scratch_rows = scratch_rows;
    a.num_item = num_item; a.n_users = n_users; a.n_pairs = n_pairs; a.min_count = (uint32_t)min_count; a.slots = slots;
    const int rc = ig_check("pmgt_item_graph_count", a, false);
    if (rc) return rc;
    return ig_launch<false>(a, stream);
}

int pmgt_item_graph_fill(const int64_t* item_ptr, const int32_t* item_users, const int64_t* user_ptr, const int32_t* user_items,
                         const int64_t* work, int64_t num_item, int64_t n_users, int64_t n_pairs, int64_t min_count, int slots,
                         const uint32_t* deg_flags, const int64_t* row_ptr, const int32_t* node_of_item, int64_t total, int32_t* indices,
                         int32_t* counts, uint32_t* scratch, int64_t scratch_rows, void* stream) {
    PMGT_CHECK(min_count >= 1 && min_count <= 0x7FFFFFFFLL, -2, "pmgt_item_graph_fill: min_count = %lld outside [1, 2^31 - 1]", (long long)min_count);
    ItemGraphArgs a = {};
    a.item_ptr = item_ptr; a.item_users = item_users; a.user_ptr = user_ptr; a.user_items = user_items; a.work = work;
    a.deg_flags = const_cast<uint32_t*>(deg_flags); a.row_ptr = row_ptr; a.node_of_item = node_of_item; a.indices = indices; a.counts = counts;
    a.scratch = scratch; a.scratch_rows = scratch_rows; a.total = total;
    a.num_item = num_item; a.n_users = n_users; a.n_pairs = n_pairs; a.min_count = (uint32_t)min_count; a.slots = slots;
    const int rc = ig_check("pmgt_item_graph_fill", a, true);
    if (rc) return rc;
    return ig_launch<true>(a, stream);
}

}  // extern "C"
