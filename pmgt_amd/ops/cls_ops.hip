// The two-way glue between the encoder and a head that is trained with it (pmgt_op_cls_gather / pmgt_op_cls_scatter of include/pmgt_ops.h;
// the reference: `self.bert(...)[0][:, 0]` and autograd's gradient of that slice, pmgt/pmgt_ncf/models.py:86-89):
//   gather    x [n][d] fp32 = the CLS state (token 0) of every sequence of last_hidden [n][S][d] in the engine dtype
//   scatter   d_last [n][S][d] in the engine dtype, written WHOLE: token 0 of sequence p = d_item[p] (fp32 -> bf16 round to nearest even),
//             every other element +0.0 -- the encoder's backward reads the whole tensor, and no memset launch precedes this one
// One launch each, grid-stride, a thread moves 8 consecutive elements with 16-byte accesses when d is a multiple of 8 and the pointers are
// 16-byte aligned (every row then starts on a 16-byte boundary in both dtypes); any other d goes element by element.  Kept out of csrc/
// for ncf_score.hip's reason: the measured pre-training step launches nothing of this.
#include "../../include/pmgt_ops.h"
#include "../csrc/common.h"

namespace pmgt {

static constexpr int CLS_THREADS = 256, CLS_MAX_BLOCKS = 8192;

__device__ __forceinline__ void load8(const float* p, f32x4& a, f32x4& b) { a = *(const f32x4*)p, b = *(const f32x4*)(p + 4); }
__device__ __forceinline__ void load8(const bf16* p, f32x4& a, f32x4& b) {
    const bf16x8 v = *(const bf16x8*)p;
    a = f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
    b = f32x4{(float)v[4], (float)v[5], (float)v[6], (float)v[7]};
}
__device__ __forceinline__ void store8(float* p, const f32x4& a, const f32x4& b) { *(f32x4*)p = a, *(f32x4*)(p + 4) = b; }
__device__ __forceinline__ void store8(bf16* p, const f32x4& a, const f32x4& b) {
    const bf16x8 v = {(bf16)a[0], (bf16)a[1], (bf16)a[2], (bf16)a[3], (bf16)b[0], (bf16)b[1], (bf16)b[2], (bf16)b[3]};
    *(bf16x8*)p = v;
}

// VEC: one thread per 8 columns of a row (d % 8 == 0); else one thread per element
template <typename T, bool VEC>
__global__ __launch_bounds__(CLS_THREADS) void cls_gather_kernel(const T* __restrict__ last, int64_t n, int S, int d, float* __restrict__ x) {
    const int per = VEC ? d >> 3 : d;                        // work items per row
    const int64_t total = n * per, stride = (int64_t)gridDim.x * CLS_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * CLS_THREADS + threadIdx.x; i < total; i += stride) {
        const int64_t p = i / per;
        const int c = (int)(i - p * per) * (VEC ? 8 : 1);
        const T* src = last + p * S * d + c;                 // token 0 of sequence p
        if constexpr (VEC) {
            f32x4 a, b;
            load8(src, a, b);
            store8(x + p * d + c, a, b);
        } else {
            x[p * d + c] = to_f<T>(src[0]);
        }
    }
}

template <typename T, bool VEC>
__global__ __launch_bounds__(CLS_THREADS) void cls_scatter_kernel(const float* __restrict__ d_item, int64_t n, int S, int d, T* __restrict__ d_last) {
    const int per = VEC ? d >> 3 : d;
    const int64_t total = n * S * per, stride = (int64_t)gridDim.x * CLS_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * CLS_THREADS + threadIdx.x; i < total; i += stride) {
        const int64_t row = i / per;                         // token row p * S + s
        const int c = (int)(i - row * per) * (VEC ? 8 : 1);
        const int64_t p = row / S;
        const bool cls = row - p * S == 0;
        if constexpr (VEC) {
            f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
            if (cls) load8(d_item + p * d + c, a, b);
            store8(d_last + row * d + c, a, b);
        } else {
            d_last[row * d + c] = from_f<T>(cls ? d_item[p * d + c] : 0.f);
        }
    }
}

static int cls_check(const char* who, int dtype, const void* a, const void* b, int64_t n, int S, int d) {
    PMGT_CHECK(dtype == PMGT_DTYPE_F32 || dtype == PMGT_DTYPE_BF16, -2, "%s: dtype %d is neither PMGT_DTYPE_F32 nor PMGT_DTYPE_BF16", who, dtype);
    PMGT_CHECK(a && b, -2, "%s: NULL buffer", who);
    PMGT_CHECK(n >= 1 && S >= 1 && d >= 1 && n <= (1LL << 40) / S / d, -2, "%s: n = %lld, S = %d, d = %d: each at least 1 and n S d at most 2^40", who,
               (long long)n, S, d);
    return 0;
}

static unsigned cls_blocks(int64_t items) { return (unsigned)std::min<int64_t>(CLS_MAX_BLOCKS, cdiv64(items, CLS_THREADS)); }

template <typename T>
static int cls_gather(const T* last, int64_t n, int S, int d, float* x, hipStream_t st) {
    const bool vec = d % 8 == 0 && (((uintptr_t)last | (uintptr_t)x) & 15) == 0;
    if (vec) hipLaunchKernelGGL((cls_gather_kernel<T, true>), dim3(cls_blocks(n * (d / 8))), dim3(CLS_THREADS), 0, st, last, n, S, d, x);
    else hipLaunchKernelGGL((cls_gather_kernel<T, false>), dim3(cls_blocks(n * d)), dim3(CLS_THREADS), 0, st, last, n, S, d, x);
    PMGT_LAUNCH_OK();
    return 0;
}

template <typename T>
static int cls_scatter(const float* d_item, int64_t n, int S, int d, T* d_last, hipStream_t st) {
    const bool vec = d % 8 == 0 && (((uintptr_t)d_item | (uintptr_t)d_last) & 15) == 0;
    if (vec) hipLaunchKernelGGL((cls_scatter_kernel<T, true>), dim3(cls_blocks(n * S * (d / 8))), dim3(CLS_THREADS), 0, st, d_item, n, S, d, d_last);
    else hipLaunchKernelGGL((cls_scatter_kernel<T, false>), dim3(cls_blocks(n * S * d)), dim3(CLS_THREADS), 0, st, d_item, n, S, d, d_last);
    PMGT_LAUNCH_OK();
    return 0;
}

}  // namespace pmgt

using namespace pmgt;

extern "C" {

int pmgt_op_cls_gather(int dtype, const void* last_hidden, int64_t n, int S, int d, float* x, void* stream) {
    if (int rc = cls_check("pmgt_op_cls_gather", dtype, last_hidden, x, n, S, d)) return rc;
    if (dtype == PMGT_DTYPE_BF16) return cls_gather<bf16>((const bf16*)last_hidden, n, S, d, x, (hipStream_t)stream);
    return cls_gather<float>((const float*)last_hidden, n, S, d, x, (hipStream_t)stream);
}

int pmgt_op_cls_scatter(int dtype, const float* d_item, int64_t n, int S, int d, void* d_last, void* stream) {
    if (int rc = cls_check("pmgt_op_cls_scatter", dtype, d_item, d_last, n, S, d)) return rc;
    if (dtype == PMGT_DTYPE_BF16) return cls_scatter<bf16>(d_item, n, S, d, (bf16*)d_last, (hipStream_t)stream);
    return cls_scatter<float>(d_item, n, S, d, (float*)d_last, (hipStream_t)stream);
}

}  // extern "C"
