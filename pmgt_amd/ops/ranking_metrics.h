// Ranking metrics on the device (ranking_metrics.hip): the workspace layout of pmgt_rank_* (include/pmgt_capi.h) and its limits.
// Host-visible parts only; the kernels live in ranking_metrics.hip.  The sort key of a score is eval_key() of eval_metrics.h.
#pragma once
#include "eval_metrics.h"

namespace pmgt {

static constexpr int RANK_THREADS = 256, RANK_WAVES = RANK_THREADS / 64;      // one workgroup per user row
static constexpr int RANK_MAX_ROW = PMGT_RANK_MAX_ROW, RANK_MAX_K = PMGT_RANK_MAX_K, RANK_MAX_KS = PMGT_RANK_MAX_KS;
static constexpr int64_t RANK_MAX_USERS = (int64_t)1 << 22;
static constexpr int64_t RANK_HEADER_BYTES = PMGT_RANK_HEADER_BYTES;
static constexpr int RANK_TABLE_CHUNK = 128;      // table entries one upload launch carries in its kernel arguments (2 KiB)

// flag bits of a user record
static constexpr uint32_t RANK_FLAG_NAN = 1u, RANK_FLAG_EMPTY = 2u, RANK_FLAG_UNWRITTEN = 4u;      // the last: set by reset, cleared by append

// the settings reset() leaves on the device: every later launch reads them there
// (the record arrays are placed by n_k, which append and reduce do not take: a launch that finds no valid block here -- no reset yet, or a
// reset for another max_users -- writes nothing)
struct RankConfig {
    int64_t max_users;
    uint32_t magic;             // RANK_MAGIC once reset has run
    int n_k;
    int max_k;                  // ks[n_k - 1]
    int ks[RANK_MAX_KS];
    int reserved[3];
};
static_assert(sizeof(RankConfig) == 48, "RankConfig is 48 bytes of the workspace");
static constexpr uint32_t RANK_MAGIC = 0x4B4E4152u;      // "RANK"

struct RankWorkspace {
    // header (PMGT_RANK_HEADER_BYTES), written by reduce: fp64 [0..3] sum of ndcg per k, [4..7] sum of recall per k, [8] sum of the per-user
    // losses; uint64 [9] n_users, [10] users with a NaN, [11] users without a positive, [12] slots no append wrote; [13..15] reserved
    double* sums;
    unsigned long long* u;      // the same sixteen words as uint64
    RankConfig* cfg;
    double* disc;               // [RANK_MAX_K]
    double* idcg;               // [RANK_MAX_K]
    double* ndcg;               // [n_k][capr]   user records, slot order
    double* recall;             // [n_k][capr]
    float* loss;                // [capr]
    int32_t* n_pos;             // [capr]
    uint32_t* flags;            // [capr]
    int64_t capr;
    int64_t bytes;
};

__host__ __device__ static inline RankWorkspace rank_carve(void* ws, int64_t max_users, int n_k) {
    const int64_t capr = (max_users + 63) / 64 * 64;
    char* p = (char*)ws;
    RankWorkspace w;
    w.sums = (double*)p;
    w.u = (unsigned long long*)p;
    p += RANK_HEADER_BYTES;
    w.cfg = (RankConfig*)p;    p += sizeof(RankConfig);
    w.disc = (double*)p;       p += RANK_MAX_K * 8;
    w.idcg = (double*)p;       p += RANK_MAX_K * 8;
    w.ndcg = (double*)p;       p += (int64_t)n_k * capr * 8;
    w.recall = (double*)p;     p += (int64_t)n_k * capr * 8;
    w.loss = (float*)p;        p += capr * 4;
    w.n_pos = (int32_t*)p;     p += capr * 4;
    w.flags = (uint32_t*)p;    p += capr * 4;
    w.capr = capr;
    w.bytes = p - (char*)ws;
    return w;
}

}  // namespace pmgt
