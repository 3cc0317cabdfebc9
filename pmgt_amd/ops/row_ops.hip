// Single-kernel entry points (include/pmgt_ops.h) of the row kernels of the training step: the embedding mix, the per-node segment sums,
// the loss heads and the weight mirror (the optimizer's entries: optimizer_step.hip).  Host code only: each entry fills the argument struct
// and calls the host function the engine calls, so a test sees the engine's own dispatch.  (Kept out of csrc/: bench.py fingerprints the
// kernel sources there, and these entries launch nothing of their own.)
#include <vector>

#include "../../include/pmgt_ops.h"
#include "../csrc/loss.h"
#include "../csrc/optim.h"
#include "../csrc/rowops.h"
#include "../csrc/segsum.h"

using namespace pmgt;

extern "C" {

static EmbedMix mk_embed(const pmgt_embed_args* a) {
    EmbedMix m;
    m.M = a->M; m.S = a->S; m.d = a->d; m.nf = a->nf; m.E = a->E; m.e_rows = a->e_rows; m.phase = a->phase; m.dF_f32 = a->dF_f32 != 0;
    m.Wa = a->Wa; m.ba = a->ba; m.pos = a->pos; m.role = a->role; m.gamma = a->gamma; m.beta = a->beta; m.eps = a->eps;
    m.a = a->a; m.pre = a->pre; m.stats = a->stats; m.h0 = a->h0;
    m.drop = DropCfg{a->rng, a->rng ? a->drop_p : 0.f, a->drop_site};
    m.dh0 = a->dh0; m.dE = a->dE; m.dF = a->dF; m.part = a->part;
    return m;
}
int pmgt_op_embed_mix_fwd(const pmgt_embed_args* a, void* stream) {
    PMGT_CHECK(a && a->phase >= 0 && a->phase <= 2, -2, "pmgt_op_embed_mix_fwd: phase must be 0, 1 or 2");
    const EmbedMix m = mk_embed(a);
    if (a->dtype == PMGT_DTYPE_BF16) return embed_mix_fwd<bf16>(m, (hipStream_t)stream);
    return embed_mix_fwd<float>(m, (hipStream_t)stream);
}
int pmgt_op_embed_mix_bwd(const pmgt_embed_args* a, void* stream) {
    PMGT_CHECK(a && a->phase >= 0 && a->phase <= 2, -2, "pmgt_op_embed_mix_bwd: phase must be 0, 1 or 2");
    const EmbedMix m = mk_embed(a);
    if (a->dtype == PMGT_DTYPE_BF16) return embed_mix_bwd<bf16>(m, (hipStream_t)stream);
    return embed_mix_bwd<float>(m, (hipStream_t)stream);
}
int pmgt_op_embed_part_elems(int d, int nf) { return embed_part_elems(d, nf); }
int pmgt_op_embed_bwd_parts(int M) { return embed_bwd_parts(M); }
int pmgt_op_pos_role_finish(const float* possum, int S, int d, int max_pos, float* dpos, float* drole, int accumulate, void* stream) {
    return pos_role_finish(possum, S, d, max_pos, dpos, drole, accumulate != 0, (hipStream_t)stream);
}

int64_t pmgt_op_seg_part_elems(int M, int cols) { return seg_part_elems(M, cols); }
int pmgt_op_seg_sum(int in_dtype, int out_dtype, const void* src, int64_t ld, const uint32_t* skeys, const uint32_t* perm, const int* seg_off,
                    int M, int n_rows, int cols, void* out, float* part, void* stream) {
    const hipStream_t st = (hipStream_t)stream;
    if (in_dtype == PMGT_DTYPE_F32 && out_dtype == PMGT_DTYPE_F32)
        return seg_sum<float, float>((const float*)src, ld, skeys, perm, seg_off, M, n_rows, cols, (float*)out, part, st);
    if (in_dtype == PMGT_DTYPE_BF16 && out_dtype == PMGT_DTYPE_BF16)
        return seg_sum<bf16, bf16>((const bf16*)src, ld, skeys, perm, seg_off, M, n_rows, cols, (bf16*)out, part, st);
    PMGT_CHECK(in_dtype == PMGT_DTYPE_BF16 && out_dtype == PMGT_DTYPE_F32, -2, "pmgt_op_seg_sum: dtype pair (%d, %d) is not built", in_dtype,
               out_dtype);
    return seg_sum<bf16, float>((const bf16*)src, ld, skeys, perm, seg_off, M, n_rows, cols, (float*)out, part, st);
}

int pmgt_op_pair_offsets(const int64_t* num_pairs, int B, int* off, void* stream) {
    return pair_offsets(num_pairs, B, off, (hipStream_t)stream);
}
int pmgt_op_nfr_compact(const int64_t* tgt_full, int B, int S, int seq_off, int64_t* rows, int64_t* tids, int* count, void* stream) {
    return nfr_compact(tgt_full, B, S, seq_off, rows, tids, count, (hipStream_t)stream);
}
int pmgt_op_nfr_generate(const int64_t* ids, int B, int S, int n_nodes, float random_ratio, float mask_ratio, const uint64_t* rng,
                         int64_t* masked_ids, int64_t* tgt_full, void* stream) {
    PMGT_CHECK(ids && rng && masked_ids && tgt_full && B > 0 && S > 0 && n_nodes > 0, -2, "pmgt_op_nfr_generate: NULL or empty argument");
    return nfr_generate(ids, B, S, n_nodes, random_ratio, mask_ratio, rng, masked_ids, tgt_full, (hipStream_t)stream);
}
int pmgt_op_build_need_rows(int B, int P, int S, const int64_t* nfr_rows, const int* nfr_count, int64_t* rows, int* count, int* inv,
                            int64_t n_tokens, void* stream) {
    PMGT_CHECK(nfr_rows && nfr_count && rows && count && B > 0 && P >= 0 && S > 0, -2, "pmgt_op_build_need_rows: NULL or empty argument");
    return build_need_rows(B, P, S, nfr_rows, nfr_count, rows, count, (hipStream_t)stream, inv, n_tokens);
}
int pmgt_op_gsr(int dtype, const void* h, void* dh, int B, int S, int d, int64_t cls_stride, const int* off, const float* labels,
                float* logits, float* loss_part, void* stream) {
    GsrArgs g;
    g.h = h; g.dh = dh; g.B = B; g.S = S; g.d = d; g.cls_stride = cls_stride; g.off = off; g.labels = labels; g.logits = logits;
    g.loss_part = loss_part;
    if (dtype == PMGT_DTYPE_BF16) return gsr_fwd_bwd<bf16>(g, (hipStream_t)stream);
    return gsr_fwd_bwd<float>(g, (hipStream_t)stream);
}
int pmgt_op_nfr_diff_parts(int cap) { return nfr_diff_parts(cap); }
int pmgt_op_nfr_diff(int dtype, void* pred, const int64_t* tids, const int* count, int cap, int nf, const int* F, const void* const* tables,
                     int tables_f8, const float* scales, float* sse_part, void* stream) {
    PMGT_CHECK(nf >= 1 && nf <= MAX_FEATS && F && tables, -2, "pmgt_op_nfr_diff: %d modalities (1 .. %d)", nf, MAX_FEATS);
    NfrDiffArgs a;
    a.pred = pred; a.tids = tids; a.count = count; a.cap = cap; a.nf = nf; a.tables_f8 = tables_f8 != 0; a.sse_part = sse_part;
    for (int m = 0; m < nf; ++m) { a.F[m] = F[m]; a.table[m] = tables[m]; a.scale[m] = scales ? scales[m] : 1.f; }
    if (dtype == PMGT_DTYPE_BF16) return nfr_diff<bf16>(a, (hipStream_t)stream);
    return nfr_diff<float>(a, (hipStream_t)stream);
}
int pmgt_op_loss_finish(const float* gsr_part, int B, const float* sse_part, int nparts, const int* count, int nf, const int* F, int with_nfr,
                        float* out, int* count_out, void* stream) {
    PMGT_CHECK(nf >= 1 && nf <= MAX_FEATS && F, -2, "pmgt_op_loss_finish: %d modalities (1 .. %d)", nf, MAX_FEATS);
    FeatSizes fs;
    fs.nf = nf;
    for (int m = 0; m < MAX_FEATS; ++m) fs.F[m] = m < nf ? F[m] : 0;
    return loss_finish(gsr_part, B, sse_part, nparts, count, fs, with_nfr != 0, out, (hipStream_t)stream, count_out);
}
int pmgt_op_scatter_rows(int dtype, const void* src, const int64_t* rows, const int* count, int cap, int d, void* dst, int add, void* stream) {
    if (dtype == PMGT_DTYPE_BF16) return scatter_rows<bf16>((const bf16*)src, rows, count, cap, d, (bf16*)dst, (hipStream_t)stream, add != 0);
    return scatter_rows<float>((const float*)src, rows, count, cap, d, (float*)dst, (hipStream_t)stream, add != 0);
}

static int mirror_from_host(int dtype, const float* params, void* mirror, const MirrorDesc* h, MirrorDesc* dev, int ndesc, int total_tiles,
                            hipStream_t st) {
    PMGT_HIP(hipMemcpyAsync(dev, h, sizeof(MirrorDesc) * (size_t)ndesc, hipMemcpyHostToDevice, st));
    const int rc = dtype == PMGT_DTYPE_BF16 ? build_mirror<bf16>(params, (bf16*)mirror, dev, ndesc, total_tiles, st)
                                            : build_mirror<float>(params, (float*)mirror, dev, ndesc, total_tiles, st);
    if (rc) return rc;
    PMGT_HIP(hipStreamSynchronize(st));       // the descriptors are freed on return
    return 0;
}
int pmgt_op_mirror(int dtype, const float* params, void* mirror, const pmgt_mirror_desc* desc, int ndesc, int total_tiles, void* stream) {
    PMGT_CHECK(desc && ndesc > 0, -2, "pmgt_op_mirror: no descriptors");
    std::vector<MirrorDesc> h((size_t)ndesc);
    for (int k = 0; k < ndesc; ++k) {
        const pmgt_mirror_desc& s = desc[k];
        h[k] = MirrorDesc{s.src, s.rows, s.cols, s.dst, s.dst_t, s.dst_t_hm, s.hm_d, s.hm_dh, s.tile_start};
    }
    const hipStream_t st = (hipStream_t)stream;
    MirrorDesc* dev = nullptr;
    PMGT_HIP(hipMalloc(&dev, sizeof(MirrorDesc) * (size_t)ndesc));
    const int rc = mirror_from_host(dtype, params, mirror, h.data(), dev, ndesc, total_tiles, st);
    if (rc) (void)hipStreamSynchronize(st);          // (the launch may be queued behind a failed step: free only when it is done)
    (void)hipFree(dev);
    return rc;
}

}  // extern "C"
