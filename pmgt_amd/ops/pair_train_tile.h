// What the kernels that TRAIN the pair heads share, stated once: ncf_train.hip (the head of PMGT_NCF over an item table or per-pair item
// rows), ncf_model_train.hip (the stand-alone NCF class: LayerNorm layers, kind GMF) and dcn_train.hip (the Deep & Cross Network).  fp32 end
// to end on the exact f32-input MFMA (v_mfma_f32_32x32x2_f32), no atomic anywhere: every sum has one fixed order, and the bits of every entry
// are pinned by tests/golden/pair_train_bits.json.
//
// EVERYTHING IS PAIR-MAJOR.  Activations, pre-activation gradients and per-pair embedding gradients sit in the caller's workspace as plain
// row-major matrices, one row per pair.  The three products are then
//   forward   Y^T [out, pair] = W [out, in] X^T          A = W[m][k]: 16 contiguous k per lane (4 x 16-byte loads), B = X[pair][k]: the same
//   data      dX^T [in, pair] = W^T [in, out] dZ^T       A = W[k][m]: one coalesced row segment per k-step,          B = dZ[pair][k]: 16 per lane
//   weight    dW [out, in]    = dZ^T [out, pair] X       A = dZ[pair][m], B = X[pair][c]: both one coalesced row segment per k-step
// with the PAIR on the lane in the first two (result register g of lane half h = feature rho(g) + 4 h, so a lane stores four 16-byte pieces
// of its pair's row) and the pairs as the contraction index of the third.  A 32-wide chunk of k is split 16 | 16 between the lane halves:
// k-step s multiplies k0 + s (half 0) and k0 + 16 + s (half 1).  Widths below 32 are zero-padded by the guards of the loads.  A tile is 32
// pairs a workgroup of 4 waves; the waves share out the 32-feature blocks of a product.
//
// THE ROLES a file's two launches take from here (block ranges by index; the tile bodies, the LayerNorm row work, the `cols` roles and the
// cross net stay with each file):
//   rank    launch 1: the position of every pair in the STABLE order by id: rank = the number of pairs with a smaller (id, pair index);
//           counted, not sorted: n <= 65 536 and the ids of a block of 256 pairs go through LDS once per 256 ranks             (pair_rank)
//   zero    launch 1: gradient rows of embedding tables, whole, as one or two ranges of 16-byte pieces                             (pair_zero)
//   weight  launch 2: one workgroup per 32 x 32 block of a layer's dW; its 4 waves take the 32-pair chunks c = w, w + 4, ... IN ORDER and
//           the four accumulators are added as (w0 + w1) + (w2 + w3).  A layer has one more block column whose B operand is the constant
//           column (1, 0, ..., 0): its column 0 is the bias gradient.  The predict / output layer is the pseudo-layer with dz = [dlogit,
//           loss of the pair]: row 0 gives its weight and bias gradient, row 1 of the constant column the loss sum         (pair_weight_block)
//   rows    launch 2: one wave per position of the stable order; the wave at the start of a run of equal ids adds the run's per-pair rows in
//           pair order and stores the table row; rows no pair touches keep the +0.0 of launch 1                 (pair_run, pair_run_sum)
//
// CONTRACTION.  ncf_train.hip is compiled with the compiler's default contraction, the other two files with it off; a pragma at file scope
// here would leak into the includer.  The products, joins, masks, the weight role and the run sums hold only MFMA, lone adds, lone
// multiplies and explicit fmaf, which contraction cannot touch.  The one block that does care, pair_bce, opens with its own
// `#pragma clang fp contract(off)` (recorded in the expressions when the template is parsed, whatever the includer's setting) and spells
// its one fused multiply-add out.
//
// Every function is inlined into its caller and takes its constants (a nullptr mask row, a key that is off) as arguments that fold there.
#pragma once
#include "ncf_head.h"

namespace pmgt {

static constexpr int PAIR_THREADS = 256, PAIR_WAVES = 4, PAIR_TILE = 32, PAIR_ZERO_BLOCKS = 1024;

__device__ __forceinline__ float4 pair_ld4(const float* p, bool ok) {
    return ok ? *reinterpret_cast<const float4*>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ float pair_elem(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }
__device__ __forceinline__ int pair_wave_index() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }      // provably uniform
__device__ __forceinline__ DropKey pair_drop_off() { return DropKey{0u, 0u, 0u, 1.f, false}; }
__device__ __forceinline__ void pair_mul4(float4& v, const float (&m)[4]) { v.x *= m[0], v.y *= m[1], v.z *= m[2], v.w *= m[3]; }
// the shuffle butterfly of the row work, 32 | 16 | .. | 1: every lane ends with the same bits.  NOT csrc/common.h's wave_sum, which pairs
// the lanes in another order: the bits of the LayerNorm rows are pinned to this one
__device__ __forceinline__ float pair_wave_sum(float x) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// HOW A PRODUCT'S k-STEPS ARE SUMMED.  An MFMA chain is a k-ordered fmaf chain per output element; within a 32-wide chunk the steps run
// s = 0 .. 15 in order (forward: s = 4 j + e over the four 16-byte pieces j and their elements e), the chunks k0 = 0, 32, .. in order.
// The bias of a forward product is the initial value of accumulator 0.  All of this is part of the contract: the bits are pinned.
//   ONE    every step on one accumulator: K / 2 dependent steps.  ncf_train.hip (K <= 512 only at d = 256, where its operator test's
//          measured ratio to the fp32 formula's error reaches 2.95 of the 4 allowed) and dcn_train.hip WITHOUT dropout (up to 3.8 on its
//          own cases): the bits these entries had before the other policies existed, kept.
//   FOUR   step s adds into accumulator s & 3 (chunk after chunk, so accumulator e holds the steps 4 j + e of every chunk), joined at the
//          end as (a0 + a1) + (a2 + a3).  ncf_model_train.hip: one chain of K / 2 steps (256 at K = 512) left the widest LayerNorm model
//          3 to 5.7 x above the error of the same formula in fp32 numpy, whose sums are blocked; four chains of K / 8 come to 2.1 x at
//          most, and four independent chains keep the MFMA pipe busy.
//   BLOCK  every chunk of 32 k sums from zero on an accumulator of its own and is added to accumulator 0 whole: K / 32 + 16 additions
//          deep instead of K / 2.  dcn_train.hip WITH dropout: with ONE pair in a call nothing averages over pairs and the yardstick's fp32
//          error is that of single BLAS dot products; ONE passed 4 x on 7 of 3 936 cases under the masks.
enum class Chain { ONE, FOUR, BLOCK };

template <Chain CH> struct PairAcc {
    f32x16 a[CH == Chain::FOUR ? 4 : 1];
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int i = 0; i < (CH == Chain::FOUR ? 4 : 1); ++i)
#pragma unroll
            for (int g = 0; g < 16; ++g) a[i][g] = 0.f;
    }
    // the 16 k-steps of one chunk, av(s) and bv(s) the operands of step s
    template <class A, class B> __device__ __forceinline__ void chunk(A av, B bv) {
        if constexpr (CH == Chain::BLOCK) {
            f32x16 blk;
#pragma unroll
            for (int g = 0; g < 16; ++g) blk[g] = 0.f;
#pragma unroll
            for (int s = 0; s < 16; ++s) blk = __builtin_amdgcn_mfma_f32_32x32x2f32(av(s), bv(s), blk, 0, 0, 0);
#pragma unroll
            for (int g = 0; g < 16; ++g) a[0][g] = a[0][g] + blk[g];
        } else {
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                f32x16& acc = a[CH == Chain::FOUR ? s & 3 : 0];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av(s), bv(s), acc, 0, 0, 0);
            }
        }
    }
    // -> accumulator 0 holds the product
    __device__ __forceinline__ void join() {
        if constexpr (CH == Chain::FOUR) {
#pragma unroll
            for (int g = 0; g < 16; ++g) a[0][g] = (a[0][g] + a[1][g]) + (a[2][g] + a[3][g]);
        }
    }
    __device__ __forceinline__ float4 piece(int q) const { return make_float4(a[0][4 * q], a[0][4 * q + 1], a[0][4 * q + 2], a[0][4 * q + 3]); }
};

// out[pair][0 .. M) = [relu](W [M][K] x + bias); x = [r1[0 .. w1) ; r2[0 .. K - w1)], the lane's own pair row(s) (one source: w1 = K)
// DROP: x is multiplied by the mask of key kx as it is loaded; the result, AFTER the ReLU, by the mask of ky before the store (row = the pair)
template <Chain CH, bool RELU, bool DROP>
__device__ __forceinline__ void pair_linear(const float* __restrict__ W, const float* __restrict__ bias, int M, int K, const float* r1, int w1,
                                            const float* r2, bool valid, float* out_row, int wave, int lane, const DropKey& kx,
                                            const DropKey& ky, int pair) {
    const int p = lane & 31, h = lane >> 5;
    for (int mb = wave; mb * 32 < M; mb += PAIR_WAVES) {
        PairAcc<CH> acc;
        acc.zero();
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int f = mb * 32 + rho(g) + 4 * h;
            acc.a[0][g] = f < M ? bias[f] : 0.f;
        }
        const int m = mb * 32 + p;
        const float* wrow = W + (int64_t)m * K;
        for (int k0 = 0; k0 < K; k0 += 32) {
            float4 a[4], x[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = k0 + 16 * h + 4 * j;
                a[j] = pair_ld4(wrow + k, m < M && k < K);
                x[j] = pair_ld4(k < w1 ? r1 + k : r2 + (k - w1), valid && k < K);
                if constexpr (DROP) {
                    if (kx.on) {
                        float mk[4];
                        drop_mul4(kx, (uint32_t)pair, (uint32_t)(k >> 2), mk);
                        pair_mul4(x[j], mk);
                    }
                }
            }
            acc.chunk([&](int s) { return pair_elem(a[s >> 2], s & 3); }, [&](int s) { return pair_elem(x[s >> 2], s & 3); });
        }
        acc.join();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int f = mb * 32 + 8 * q + 4 * h;
            float4 v = acc.piece(q);
            if constexpr (RELU) v.x = relu_keep_nan(v.x), v.y = relu_keep_nan(v.y), v.z = relu_keep_nan(v.z), v.w = relu_keep_nan(v.w);
            if constexpr (DROP) {
                if (ky.on) {
                    float mk[4];
                    drop_mul4(ky, (uint32_t)pair, (uint32_t)(f >> 2), mk);
                    pair_mul4(v, mk);
                }
            }
            if (valid && f < M) *reinterpret_cast<float4*>(out_row + f) = v;
        }
    }
}

// dx[pair][c] = sum_o W[o][c] dz[pair][o] for c in [0, C), W [M][K] with C <= K; times (mask_row[c] > 0) when mask_row
// DROP: a gradient that passes mask_row is multiplied by gscale (the scale of the layer that wrote mask_row), and the result by the mask of kx
template <Chain CH, bool DROP>
__device__ __forceinline__ void pair_linear_bwd(const float* __restrict__ W, int M, int K, int C, const float* dz_row, const float* mask_row,
                                                bool valid, float* dx_row, int wave, int lane, float gscale, const DropKey& kx, int pair) {
    const int p = lane & 31, h = lane >> 5;
    for (int cb = wave; cb * 32 < C; cb += PAIR_WAVES) {
        PairAcc<CH> acc;
        acc.zero();
        const int c = cb * 32 + p;
        for (int o0 = 0; o0 < M; o0 += 32) {
            float4 z[4];
            float a[16];
#pragma unroll
            for (int j = 0; j < 4; ++j) z[j] = pair_ld4(dz_row + o0 + 16 * h + 4 * j, valid && o0 + 16 * h + 4 * j < M);
#pragma unroll
            for (int s = 0; s < 16; ++s) {
                const int o = o0 + 16 * h + s;
                a[s] = (c < C && o < M) ? W[(int64_t)o * K + c] : 0.f;
            }
            acc.chunk([&](int s) { return a[s]; }, [&](int s) { return pair_elem(z[s >> 2], s & 3); });
        }
        acc.join();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int f = cb * 32 + 8 * q + 4 * h;
            const bool ok = valid && f < C;
            float4 v = acc.piece(q);
            if (mask_row) {
                const float4 hm = pair_ld4(mask_row + f, ok);
                v.x = hm.x > 0.f ? v.x : 0.f;
                v.y = hm.y > 0.f ? v.y : 0.f;
                v.z = hm.z > 0.f ? v.z : 0.f;
                v.w = hm.w > 0.f ? v.w : 0.f;
                if constexpr (DROP) v.x *= gscale, v.y *= gscale, v.z *= gscale, v.w *= gscale;
            }
            if constexpr (DROP) {
                if (kx.on) {
                    float mk[4];
                    drop_mul4(kx, (uint32_t)pair, (uint32_t)(f >> 2), mk);
                    pair_mul4(v, mk);
                }
            }
            if (ok) *reinterpret_cast<float4*>(dx_row + f) = v;
        }
    }
}

// sig = sigmoid(z), dl = (sig - y) / n, loss = max(z, 0) - z y + log1p(exp(-|z|)) of one pair.  FUSED: max(z, 0) - z y is ONE fused
// multiply-add, fmaf(-z, y, max(z, 0)): what the build of ncf_train.hip made of the expression under the compiler's default contraction
// (v_fma_f32 in its assembly) before this block stated it; the other two files round the product first.
template <bool FUSED>
__device__ __forceinline__ void pair_bce(float z, float y, int n, float& dl, float& loss) {
#pragma clang fp contract(off)
    const float e = expf(-fabsf(z));
    const float sig = z >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
    dl = (sig - y) / (float)n;
    if constexpr (FUSED) loss = fmaf(-z, y, fmaxf(z, 0.f)) + log1pf(e);
    else loss = (fmaxf(z, 0.f) - z * y) + log1pf(e);
}

// ---- rank: entered by the whole workgroup of rank block `bid` (0 .. 2 rank_blocks: the user order, then the item order)
__device__ __forceinline__ void pair_rank(int bid, int rank_blocks, int n, const int64_t* users, const int64_t* items, int* order_u, int* order_i,
                                          int64_t (&s_ids)[PAIR_THREADS], int tid) {
    const int kind = bid / rank_blocks;
    const int64_t* ids = kind ? items : users;
    int* order = kind ? order_i : order_u;
    const int p = (bid - kind * rank_blocks) * PAIR_THREADS + tid;
    const int64_t mine = p < n ? ids[p] : 0;
    int rank = 0;
    for (int q0 = 0; q0 < n; q0 += PAIR_THREADS) {
        __syncthreads();
        s_ids[tid] = q0 + tid < n ? ids[q0 + tid] : 0;
        __syncthreads();
        const int cnt = min(PAIR_THREADS, n - q0);
        for (int j = 0; j < cnt; ++j) {
            const int64_t v = s_ids[j];
            rank += (v < mine || (v == mine && q0 + j < p)) ? 1 : 0;
        }
    }
    if (p < n) order[rank] = p;
}

// ---- zero: block `bid` of `blocks` clears vec4 16-byte pieces at base and, behind them, vec4b at base2 (TWO false: the first range only)
template <bool TWO>
__device__ __forceinline__ void pair_zero(int bid, int blocks, float* base, int64_t vec4, float* base2, int64_t vec4b, int tid) {
    float4* z = reinterpret_cast<float4*>(base);
    float4* z2 = reinterpret_cast<float4*>(base2);
    const int64_t total = vec4 + (TWO ? vec4b : 0);
    for (int64_t i = (int64_t)bid * PAIR_THREADS + tid; i < total; i += (int64_t)blocks * PAIR_THREADS) {
        if (!TWO || i < vec4) z[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        else z2[i - vec4] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// a matrix [n][w1 + w2] given by one or two row sources, each read by the pair index itself (idx NULL) or through an id list
struct PairSrc {
    const float* p1;
    const int64_t* idx1;
    int w1;
    const float* p2;
    const int64_t* idx2;
    int w2;
};

// the weight gradient of one layer
struct PairTask {
    const float* a;      // dz [n][m]
    PairSrc b;           // the layer's input [n][k]
    float* gw;           // [m][k]
    float* gb;           // [m]
    int m, col_blocks, first, predict;      // col_blocks counts the constant column's block; first: the task's first block
};

// GATHER false: no source of the kernel has an id list (the idx fields are not read)
template <bool GATHER>
__device__ __forceinline__ float pair_src_at(const PairSrc& s, int pair, int c) {
    if (c < s.w1) {
        const int64_t row = GATHER && s.idx1 ? s.idx1[pair] : pair;
        return s.p1[row * s.w1 + c];
    }
    const int64_t row = GATHER && s.idx2 ? s.idx2[pair] : pair;
    return s.p2[row * s.w2 + (c - s.w1)];
}

// ---- weight: block `bid` of the tasks' blocks: one 32 x 32 block of dW = dz^T x, the pairs in order; the predict task stores loss = v / n
// DROP: task 0, when it is a layer, gathers its B operand from the tables and applies the mask of `emb` to it, drawn again per element
template <bool DROP, bool GATHER>
__device__ __forceinline__ void pair_weight_block(const PairTask* tasks, int ntasks, int bid, int n, float* loss, const DropCfg& emb,
                                                  float (&s_acc)[PAIR_WAVES][16][64], int tid, int lane, int wave) {
    int ti = 0;
    for (int i = 1; i < ntasks; ++i)
        if (bid >= tasks[i].first) ti = i;
    const PairTask t = tasks[ti];                            // a COPY: the fields stay in scalar registers over the chunk loop, where a reference is
                                                             // read again behind every store (the argument struct is indexed by a run-time ti)
    const int local = bid - t.first, M = t.m, K = t.b.w1 + t.b.w2;
    const int mb = local / t.col_blocks, nb = local - mb * t.col_blocks;
    const bool ones = nb == t.col_blocks - 1;
    const int p = lane & 31, h = lane >> 5, m = mb * 32 + p, c = nb * 32 + p;
    DropKey kemb = pair_drop_off();
    if constexpr (DROP) {
        if (ti == 0 && !t.predict && !ones) kemb = make_drop_key(emb);
    }
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.f;
    for (int ch = wave; ch * 32 < n; ch += PAIR_WAVES) {
        float av[16], bv[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int pair = ch * 32 + 16 * h + s;
            const bool ok = pair < n;
            av[s] = (ok && m < M) ? t.a[(int64_t)pair * M + m] : 0.f;
            bv[s] = ones ? (p == 0 ? 1.f : 0.f) : ((ok && c < K) ? pair_src_at<GATHER>(t.b, pair, c) : 0.f);
            if constexpr (DROP) {
                if (kemb.on) bv[s] *= drop_mul1(kemb, (uint32_t)pair, (uint32_t)c);
            }
        }
#pragma unroll
        for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], bv[s], acc, 0, 0, 0);
    }
#pragma unroll
    for (int g = 0; g < 16; ++g) s_acc[wave][g][lane] = acc[g];
    __syncthreads();
    const int gq = tid >> 6;
#pragma unroll
    for (int gg = 0; gg < 4; ++gg) {
        const int g = gq * 4 + gg;
        const float v = (s_acc[0][g][lane] + s_acc[1][g][lane]) + (s_acc[2][g][lane] + s_acc[3][g][lane]);
        const int mo = mb * 32 + rho(g) + 4 * h;
        if (t.predict) {
            if (mo == 0) {
                if (ones) { if (p == 0) t.gb[0] = v; }
                else if (c < K) t.gw[c] = v;
            } else if (mo == 1 && ones && p == 0) {
                loss[0] = v / (float)n;
            }
        } else if (mo < M) {
            if (ones) { if (p == 0) t.gb[mo] = v; }
            else if (c < K) t.gw[(int64_t)mo * K + c] = v;
        }
    }
}

// ---- rows: the wave of block `bid` (0 .. 2 row_blocks: the user order, then the item order) at position s of its kind's stable order
struct PairRun {
    const int64_t* ids;
    const int* order;
    int64_t id;          // the id at position s
    int kind, s;
    bool start;          // (uniform per wave) s is inside the order and the first position of its id: this wave sums the run
};
__device__ __forceinline__ PairRun pair_run(int bid, int row_blocks, int wave, int n, const int64_t* users, const int64_t* items,
                                            const int* order_u, const int* order_i) {
    PairRun r;
    r.kind = bid / row_blocks;
    r.s = (bid - r.kind * row_blocks) * PAIR_WAVES + wave;
    r.ids = r.kind ? items : users;
    r.order = r.kind ? order_i : order_u;
    r.id = 0;
    r.start = false;
    if (r.s < n) {
        r.id = r.ids[r.order[r.s]];
        r.start = !(r.s > 0 && r.ids[r.order[r.s - 1]] == r.id);
    }
    return r;
}
// column cc of the run's per-pair rows (`sw` floats apart at src), added in pair order
__device__ __forceinline__ float pair_run_sum(const PairRun& r, int n, const float* src, int sw, int cc) {
    float sum = 0.f;
    for (int t = r.s; t < n; ++t) {
        const int pr = r.order[t];
        if (r.ids[pr] != r.id) break;
        sum += src[(int64_t)pr * sw + cc];
    }
    return sum;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
// one p of a dropout, `name` or `name[index]` (index < 0: no index): refused when outside [0, 1) (a NaN fails both comparisons); > 0 sets *on
inline int pair_check_p(const char* who, const char* name, int index, float p, bool* on) {
    const bool ok = p >= 0.f && p < 1.f;
    PMGT_CHECK(ok || index >= 0, -2, "%s: %s = %g outside [0, 1)", who, name, (double)p);
    PMGT_CHECK(ok, -2, "%s: %s[%d] = %g outside [0, 1)", who, name, index, (double)p);
    *on = *on || p > 0.f;
    return 0;
}

// the rows of the two embedding tables; the pairs of a call
inline int pair_check_rows(const char* who, int64_t user_num, int64_t item_num) {
    PMGT_CHECK(user_num >= 1 && user_num <= 0x7FFFFFFELL, -2, "%s: user_num = %lld outside [1, 2^31 - 2]", who, (long long)user_num);
    PMGT_CHECK(item_num >= 1 && item_num <= 0x7FFFFFFELL, -2, "%s: item_num = %lld outside [1, 2^31 - 2]", who, (long long)item_num);
    return 0;
}
inline int pair_check_n(const char* who, int64_t n, int max_pairs) {
    PMGT_CHECK(n >= 1 && n <= max_pairs, -2, "%s: n = %lld pairs outside [1, %d]", who, (long long)n, max_pairs);
    return 0;
}
// the ids (8 bytes) and the small float buffers (4 bytes) of every entry; NULL passes
inline int pair_check_small(const char* who, const int64_t* users, const int64_t* items, const float* labels, const float* loss, const float* logits) {
    PMGT_CHECK((((uintptr_t)labels | (uintptr_t)loss | (uintptr_t)logits) & 3) == 0 && (((uintptr_t)users | (uintptr_t)items) & 7) == 0, -2,
               "%s: misaligned buffer", who);
    return 0;
}

// after every p of a call: a dropout that is on needs the device {seed, step} pair
inline int pair_check_rng(const char* who, bool drop_on, const uint64_t* rng) {
    PMGT_CHECK(!drop_on || (rng && ((uintptr_t)rng & 7) == 0), -2, "%s: dropout needs the device {seed, step} pair, 8-byte aligned", who);
    return 0;
}
// p_emb and p_layer[0 .. L) of a pmgt_ncf_dropout (drop NULL: none) -> *dr, *drop_on (every p 0: the instantiations without dropout)
inline int pair_check_ncf_dropout(const char* who, const pmgt_ncf_dropout* drop, int L, pmgt_ncf_dropout* dr, bool* drop_on) {
    *dr = pmgt_ncf_dropout{};
    *drop_on = false;
    if (!drop) return 0;
    dr->rng = drop->rng, dr->p_emb = drop->p_emb;
    if (int rc = pair_check_p(who, "p_emb", -1, dr->p_emb, drop_on)) return rc;
    for (int l = 0; l < L; ++l) {
        dr->p_layer[l] = drop->p_layer[l];
        if (int rc = pair_check_p(who, "p_layer", l, dr->p_layer[l], drop_on)) return rc;
    }
    return pair_check_rng(who, *drop_on, dr->rng);
}

// appends the weight task of one layer (dz [n][m] against the input b [n][k]; the pseudo-layer has m = 2: one block row) and advances *first
inline void pair_add_task(PairTask* tasks, int* ntasks, int* first, const float* dz, int m, const PairSrc& b, float* gw, float* gb, bool predict) {
    PairTask& t = tasks[(*ntasks)++];
    t.a = dz, t.b = b, t.gw = gw, t.gb = gb;
    t.m = m;
    t.col_blocks = (b.w1 + b.w2 + 31) / 32 + 1;
    t.first = *first;
    t.predict = predict ? 1 : 0;
    *first += (m + 31) / 32 * t.col_blocks;
}

}  // namespace pmgt
