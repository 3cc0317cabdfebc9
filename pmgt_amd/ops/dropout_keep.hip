// Test surface (include/pmgt_ops.h): the keep decisions of the counter-based dropout RNG (csrc/common.h: make_drop_key + drop_keep4) for a
// [rows, cols] site, written as bytes -- what a CPU restatement of the hash is compared with, bit for bit, before it is trusted to build the
// reference masks of the dropout-on parity tests.  Kept out of csrc/: the step launches nothing of this, and bench.py fingerprints the kernel
// sources there.
#include "../../include/pmgt_ops.h"
#include "../csrc/common.h"

namespace pmgt {

// one thread per (row, column group of 4): the same (row, cg) indexing every dropout-bearing kernel uses
__global__ __launch_bounds__(256) void dropout_keep_kernel(DropCfg c, int rows, int cols, int ncg, uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)rows * ncg) return;
    const uint32_t r = (uint32_t)(i / ncg), cg = (uint32_t)(i % ncg);
    const DropKey k = make_drop_key(c);
    bool kp[4] = {true, true, true, true};
    if (k.on) drop_keep4(k, r, cg, kp);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int col = 4 * (int)cg + e;
        if (col < cols) out[(int64_t)r * cols + col] = kp[e] ? 1 : 0;
    }
}

}  // namespace pmgt

using namespace pmgt;

extern "C" int pmgt_op_dropout_keep(const uint64_t* rng, float p, uint32_t site, int rows, int cols, uint8_t* out, void* stream) {
    PMGT_CHECK(rows > 0 && cols > 0 && out, -2, "pmgt_op_dropout_keep: empty output");
    PMGT_CHECK(rng || !(p > 0.f), -2, "pmgt_op_dropout_keep: p > 0 needs the {seed, step} pair");
    const int ncg = cdiv(cols, 4);
    const int64_t blocks = cdiv64((int64_t)rows * ncg, 256);
    PMGT_CHECK(blocks <= 0x7FFFFFFF, -2, "pmgt_op_dropout_keep: %d x %d is too large for one launch", rows, cols);
    hipLaunchKernelGGL(dropout_keep_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, DropCfg{rng, p, site}, rows, cols, ncg, out);
    PMGT_LAUNCH_OK();
    return 0;
}
