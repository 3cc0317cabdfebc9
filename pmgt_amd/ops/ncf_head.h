// What the scoring and the training kernels of the pair heads share: the accumulator and register order of the 32 x 32 MFMA block, the ReLU,
// the covered heads, the dropout sites of the trained head and of the DCN.  Included through ncf_score_tile.h (the scoring tower of
// ncf_score.hip, ncf_model_score.hip, dcn_score.hip) and pair_train_tile.h (the pair-major training tile of ncf_train.hip,
// ncf_model_train.hip, dcn_train.hip); item_sim.hip takes the block order alone.
#pragma once
#include "../csrc/common.h"
#include "../../include/pmgt_capi.h"

namespace pmgt {

typedef __attribute__((ext_vector_type(16))) float f32x16;
static constexpr int NCF_MAX_D = 256;      // the widest layer-0 half: d = factor_num * 2^(num_layers - 1)
// the dropout sites of the trained head (DropCfg.site; pmgt_ncf_train_grad_dropout of include/pmgt_capi.h, mirrored in _lib.py): the
// concatenated [user ; item] input, the GMF product, and layer l's output = NCF_SITE_LAYER + l.  Row = the pair's index within the call, column = the feature.
static constexpr uint32_t NCF_SITE_EMB = 64, NCF_SITE_GMF = 65, NCF_SITE_LAYER = 72;
// the dropout sites of the Deep & Cross Network (dcn_train.hip; pmgt_dcn_train_grad_dropout of include/pmgt_capi.h, mirrored in _lib.py): the
// concatenated [user ; item] input, deep layer l's Linear output = DCN_SITE_DEEP + l, cross layer c's product x0 s_c = DCN_SITE_CROSS + c
static constexpr uint32_t DCN_SITE_EMB = 64, DCN_SITE_DEEP = 72, DCN_SITE_CROSS = 80;

// relu that keeps a NaN (fmaxf would return 0 and hide a broken table from the NaN check of the selection)
__device__ __forceinline__ float relu_keep_nan(float x) { return x < 0.f ? 0.f : x; }
__device__ __forceinline__ int rho(int g) { return (g & 3) + 8 * (g >> 2); }

// the covered heads -> 0 and *d, or -2 with the error set in the name of the entry `who`
inline int ncf_head_check(int factor_num, int num_layers, int kind, const char* who, int* d) {
    PMGT_CHECK(factor_num == 8 || factor_num == 16 || factor_num == 32 || factor_num == 64, -2, "%s: factor_num = %d, covered: 8, 16, 32, 64", who, factor_num);
    PMGT_CHECK(num_layers >= 1 && num_layers <= PMGT_NCF_MAX_LAYERS, -2, "%s: num_layers = %d outside [1, %d]", who, num_layers, PMGT_NCF_MAX_LAYERS);
    *d = factor_num << (num_layers - 1);
    PMGT_CHECK(*d <= NCF_MAX_D, -2, "%s: d = factor_num * 2^(num_layers - 1) = %d above %d", who, *d, NCF_MAX_D);
    PMGT_CHECK(kind == PMGT_NCF_MLP || kind == PMGT_NCF_NEUMF_END, -2, "%s: unknown model kind %d", who, kind);
    return 0;
}

}  // namespace pmgt
