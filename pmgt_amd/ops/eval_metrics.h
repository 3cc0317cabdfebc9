// Validation metrics on the device (eval_metrics.hip): the workspace layout of pmgt_eval_* (include/pmgt_capi.h), the order-preserving
// sort key of a score, and the constants of the two reduce paths.  Host-visible parts only; the kernels live in eval_metrics.hip.
#pragma once
#include "../../include/pmgt_ops.h"
#include "../csrc/common.h"

namespace pmgt {

// one workgroup of EVAL_SMALL_THREADS threads sorts up to EVAL_SMALL_MAX predictions in LDS (33-bit composite (key << 1) | label as
// uint64: 32 KiB, plus the negative-prefix table, 16 KiB); more predictions take the multi-tile radix path
static constexpr int EVAL_SMALL_THREADS = 1024, EVAL_SMALL_MAX = 4096;
// multi-tile path: the tile of csrc/segsum.hip's radix sort (256 threads x 8 rounds)
static constexpr int EVAL_ROUNDS = 8, EVAL_TILE = 256 * EVAL_ROUNDS, EVAL_SLOTS = 4 * EVAL_ROUNDS;
static constexpr int64_t EVAL_MAX_CAPACITY = (int64_t)1 << 26;      // twoU < 2^53: the host's one division sees an exact double
static constexpr int64_t EVAL_HEADER_BYTES = PMGT_EVAL_HEADER_BYTES;

struct EvalWorkspace {
    // header (PMGT_EVAL_HEADER_BYTES): [0] fp64 loss accumulator, uint64 [1] twoU, [2] n_pos, [3] n_neg, [4] NaN scores, [5] n of the last reduce
    double* acc;
    unsigned long long* u;      // the same eight words as uint64
    uint32_t* keys;             // [capr] slot order
    float* scores;              // [capr]
    uint8_t* labels;            // [capr]
    // scratch of the multi-tile reduce: two (key, label) buffers the four radix passes alternate between, the [tile][digit] count table,
    // its column totals, and the per-tile negative counts; the negative-prefix table reuses keys_b once the sort has left it
    uint32_t *keys_b, *keys_c;
    uint8_t *labels_b, *labels_c;
    uint32_t *hist, *coltot, *tileneg;
    int64_t bytes;
};

static inline int64_t eval_round_capacity(int64_t capacity) { return (capacity + 255) / 256 * 256; }
static inline int eval_tiles(int64_t n) { return (int)((n + EVAL_TILE - 1) / EVAL_TILE); }

static inline EvalWorkspace eval_carve(void* ws, int64_t capacity) {
    const int64_t capr = eval_round_capacity(capacity);
    const int64_t tiles = capacity > EVAL_SMALL_MAX ? eval_tiles(capacity) : 0;      // a small workspace carries no radix scratch
    char* p = (char*)ws;
    EvalWorkspace w;
    w.acc = (double*)p;
    w.u = (unsigned long long*)p;
    p += EVAL_HEADER_BYTES;
    w.keys = (uint32_t*)p;   p += capr * 4;
    w.scores = (float*)p;    p += capr * 4;
    w.labels = (uint8_t*)p;  p += capr;
    const int64_t sc = tiles ? capr : 0;
    w.keys_b = (uint32_t*)p;   p += sc * 4;
    w.keys_c = (uint32_t*)p;   p += sc * 4;
    w.labels_b = (uint8_t*)p;  p += sc;
    w.labels_c = (uint8_t*)p;  p += sc;
    w.hist = (uint32_t*)p;     p += tiles * 256 * 4;
    w.coltot = (uint32_t*)p;   p += (tiles ? 256 : 0) * 4;
    w.tileneg = (uint32_t*)p;  p += (tiles ? (tiles + 1 + 63) / 64 * 64 : 0) * 4;
    w.bytes = p - (char*)ws;
    return w;
}

// Order-preserving uint32 image of an fp32 score: -0.0f is folded onto +0.0f first (sklearn ties the two), then negative values have
// every bit flipped and the others the sign bit set, so unsigned order of the keys = numeric order of the scores.  NaN gets no key.
__host__ __device__ static inline uint32_t eval_key(float s) {
    uint32_t b = __builtin_bit_cast(uint32_t, s);
    if (s == 0.f) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

}  // namespace pmgt
