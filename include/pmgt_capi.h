/*
 * pmgt_capi.h — C ABI of the MI355X-native PMGT pre-training engine (libpmgt_hip.so) and of the
 * host MCNSampling library (libpmgt_sampler.so).
 *
 * The reference (uoo723/PMGT) is pure Python and has no FFI of its own; this ABI is what a
 * maintainer binds (ctypes) behind the reference's Python surface.  Each entry
 * point names the reference interface it replaces (paths relative to the reference root).
 *
 * Conventions: plain pointers and sizes only (no torch types); all tensor memory is owned by the
 * caller (device pointers unless stated); row-major contiguous; int64 ids, fp32 masks, nn.Linear
 * weights as [out, in]; every call is asynchronous on the given hipStream_t (passed as void*), never
 * synchronises, never throws; returns 0 or a negative code, message via pmgt_last_error().
 */
#ifndef PMGT_CAPI_H
#define PMGT_CAPI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PMGT_DTYPE_F32 0  /* parity mode: fp32 storage, exact-fp32 MFMA (v_mfma_f32_16x16x4_f32) */
#define PMGT_DTYPE_BF16 1 /* perf mode: bf16 activations/weight copies, fp32 accumulate + master weights */
/* fp8 mode (BASELINE.json config 5): the bf16 engine with OCP e4m3 where the north star names it -- frozen feature tables
 * stored as e4m3 (one scale per table), feature-projection and Q|K|V|C projections on the fp8 MFMA
 * (v_mfma_scale_f32_16x16x128_f8f6f4, unit block scales) with
 * weights quantised per output channel and activations per row; every other tensor, the attention, the backward GEMMs and
 * the optimizer as in PMGT_DTYPE_BF16. */
#define PMGT_DTYPE_FP8 2

/* Modalities: PMGTEmbeddings / PMGTNodeConstructLoss / PMGT.feat_embeddings are generic over len(feat_hidden_sizes)
 * (pmgt/pmgt/modeling_pmgt.py:163-173,195-201,549-569; pmgt/pmgt/models.py:38-54); the reference's trainer builds two
 * (visual 1536, textual 768; pmgt/pmgt/trainer.py:114-125).  The engine takes 1 .. PMGT_MAX_FEATS of them. */
#define PMGT_MAX_FEATS 4

/* Mirrors PMGTConfig (pmgt/pmgt/configuration_pmgt.py:11-41). */
typedef struct pmgt_config {
    int hidden_size;
    int num_hidden_layers;
    int num_attention_heads;
    int intermediate_size;
    int n_feats;                     /* len(feat_hidden_sizes) */
    int feat_sizes[PMGT_MAX_FEATS];  /* feat_hidden_sizes (each a multiple of 8); entries past n_feats are ignored */
    int max_position_embeddings;
    float layer_norm_eps;
    float beta;
    float hidden_dropout_prob;
    float attention_probs_dropout_prob;
    int dtype; /* PMGT_DTYPE_* */
} pmgt_config;

typedef struct pmgt_engine pmgt_engine;

const char* pmgt_last_error(void);
int pmgt_abi_version(void);

/* ---- engine lifetime & parameter layout ---------------------------------------------------------
 * Replaces PMGT.__init__ / PMGTModel.__init__ module construction (pmgt/pmgt/models.py:22-54,
 * pmgt/pmgt/modeling_pmgt.py:65-74,155-187,213-220,287-294,378-410,549-558): parameters live in ONE
 * flat fp32 buffer; pmgt_param_entry() reports where each reference-named tensor sits in it. */
pmgt_engine* pmgt_engine_create(const pmgt_config* cfg);
void pmgt_engine_destroy(pmgt_engine* e);
int64_t pmgt_param_count(const pmgt_engine* e);
int pmgt_param_num_entries(const pmgt_engine* e);
/* name: reference state_dict key (e.g. "bert.encoder.layer.0.attention.self.query.weight");
 * offset/numel in floats; rows/cols (cols = 0 for vectors); decay = 1 if AdamW weight decay applies
 * (pmgt/base_trainer.py:38-59). */
int pmgt_param_entry(const pmgt_engine* e, int index, char* name, int name_cap, int64_t* offset, int64_t* numel,
                     int* rows, int* cols, int* decay);
/* bytes of scratch the calls below need for n_seq sequences of seq_len tokens (n_targets of them targets). */
int64_t pmgt_workspace_bytes(const pmgt_engine* e, int n_seq, int seq_len, int n_targets, int training);

/* persistent device tensors owned by the caller */
typedef struct pmgt_tensors {
    float* params;       /* [pmgt_param_count] fp32 master weights */
    float* grads;        /* same shape; written (or accumulated) by pmgt_pretrain_step */
    const void* tables[PMGT_MAX_FEATS]; /* tables[m]: [n_nodes + 2, feat_sizes[m]] frozen features in the engine dtype
                                          * (PMGT.feat_embeddings, models.py:40-54); e4m3 bytes in fp8 mode */
    int64_t n_nodes;
    uint64_t* rng_state; /* device [2]: {seed, step}; drives dropout + NFR masking */
    /* PMGT_DTYPE_FP8 only: the tables are e4m3 bytes, feature value = byte value * table_scales[m] (pmgt_quantize_e4m3) */
    float table_scales[PMGT_MAX_FEATS];
} pmgt_tensors;

/* One collated batch, exactly what pmgt_collate_fn returns (pmgt/pmgt/datasets.py:186-208). */
typedef struct pmgt_batch {
    int n_targets;            /* B */
    int n_pairs;              /* sum(num_pairs) */
    int seq_len;              /* S = max_ctx_neigh + 1 */
    const int64_t* tgt_ids;   /* [B, S] */
    const float* tgt_mask;    /* [B, S] */
    const int64_t* pair_ids;  /* [P, S] (NULL with n_pairs = 0: inference) */
    const float* pair_mask;   /* [P, S] */
    const int64_t* num_pairs; /* [B] */
    const float* labels;      /* [P] */
    /* optional injected NFR masking (parity tests): masked ids and, per position, the id to
     * reconstruct (-1 = not masked).  NULL = draw on device (pmgt/pmgt/models.py:132-151). */
    const int64_t* nfr_masked_ids; /* [B, S] */
    const int64_t* nfr_targets;    /* [B, S] */
    float random_node_ratio;
    float mask_node_ratio;
} pmgt_batch;

typedef struct pmgt_outputs {
    float* loss;       /* device [3]: loss, gsr, nfr */
    float* logits;     /* device [P] prediction_logits */
    void* last_hidden; /* device [B, S, d] in the engine dtype (target sequences), nullable */
    int* nfr_count;    /* device [1], nullable: number of masked positions */
} pmgt_outputs;

#define PMGT_FLAG_TRAINING 1   /* dropout + NFR branch (module.training) */
#define PMGT_FLAG_BACKWARD 2   /* also compute parameter gradients */
#define PMGT_FLAG_ACCUMULATE 4 /* grads += instead of grads = */

/* PMGT.forward + loss.backward() of one batch (pmgt/pmgt/models.py:56-176; trainer step
 * pmgt/pmgt/trainer.py:156-160). */
int pmgt_pretrain_step(pmgt_engine* e, const pmgt_tensors* t, const pmgt_batch* b, const pmgt_outputs* o,
                       void* workspace, int64_t workspace_bytes, int flags, void* stream);

/* PMGTModel.forward on node ids (gather fused): inference/export path
 * (pmgt/pmgt/modeling_pmgt.py:80-152, pmgt/pmgt/trainer.py:153-154).  hidden_states: optional
 * [L+1, n_seq, S, d]; attn_probs: optional [L, n_seq, H, S, S] fp32 (output_attentions). */
int pmgt_encode_ids(pmgt_engine* e, const pmgt_tensors* t, const int64_t* ids, const float* mask, int n_seq,
                    int seq_len, void* last_hidden, void* hidden_states, float* attn_probs, void* workspace,
                    int64_t workspace_bytes, void* stream);
/* PMGTModel.forward(*input_feat_embeds) on already-gathered features: feats[m] = [n_seq, S, feat_sizes[m]] in the engine
 * dtype, m < n_feats (a host array of device pointers). */
int pmgt_encode_feats(pmgt_engine* e, const pmgt_tensors* t, const void* const* feats,
                      const float* mask, int n_seq, int seq_len, void* last_hidden, void* hidden_states,
                      float* attn_probs, void* workspace, int64_t workspace_bytes, void* stream);

/* PMGTModel.forward + backward for a caller that owns the head (second caller of the boundary: PMGT_NCF,
 * pmgt/pmgt_ncf/models.py:77-105 -- `self.bert(*input_feat_embeds, attention_mask=...)[0][:, 0]` followed by
 * autograd).  pmgt_encode_train runs the encoder on node ids (ids != NULL, gather fused) or on gathered features
 * (ids == NULL: feats[m] = [n_seq, S, feat_sizes[m]], engine dtype), keeps every activation in `workspace`
 * (pmgt_workspace_bytes(e, n_seq, S, 1, 1) bytes, untouched until the backward call) and snapshots the dropout
 * counter; PMGT_FLAG_TRAINING turns dropout on and advances the counter.  pmgt_encode_backward takes
 * d loss / d last_hidden_state [n_seq, S, d] (engine dtype) and leaves the gradients of every `bert.*` entry in
 * t->grads (= or += with PMGT_FLAG_ACCUMULATE; pass the same TRAINING flag); the frozen tables get none
 * (pmgt/pmgt_ncf/models.py:45-47).  `feats` is needed again only when the forward used it (NULL otherwise). */
int pmgt_encode_train(pmgt_engine* e, const pmgt_tensors* t, const int64_t* ids, const void* const* feats,
                      const float* mask, int n_seq, int seq_len, void* last_hidden, void* workspace,
                      int64_t workspace_bytes, int flags, void* stream);
int pmgt_encode_backward(pmgt_engine* e, const pmgt_tensors* t, const void* const* feats,
                         const void* d_last_hidden, int n_seq, int seq_len, void* workspace, int64_t workspace_bytes,
                         int flags, void* stream);

/* Global-norm clip + DenseSparseAdamW dense step over the flat buffers
 * (pmgt/base_trainer.py:312-315, pmgt/optimizers.py:256-270). */
typedef struct pmgt_adam {
    float* exp_avg;       /* [count] */
    float* exp_avg_sq;    /* [count] */
    const uint8_t* decay; /* [count] 1 where weight decay applies */
    float lr, weight_decay, beta1, beta2, eps;
    float max_grad_norm; /* <= 0: no clipping */
    int64_t* step;       /* device [1] */
    float* scalars;      /* device [4] out: clip coef, lr/bc1, 1/sqrt(bc2), grad norm */
    float* scratch;      /* device [1024] */
} pmgt_adam;
int pmgt_optimizer_step(pmgt_engine* e, const pmgt_tensors* t, const pmgt_adam* a, void* stream);

/* Learning-rate schedule evaluated ON THE DEVICE from the optimizer's step counter, so a captured step follows it with no
 * re-capture and no host write between replays (the reference: --scheduler-type / --scheduler-warmup, train.py:38-52, meant for
 * transformers' get_scheduler stepped once per optimizer step, pmgt/base_trainer.py:71-90,152-162).  The step that follows k
 * completed steps uses lr_t = a->lr * lambda(k) (LambdaLR's convention), lambda = the multiplier of transformers 4.11.2
 * optimization.py with the defaults get_scheduler leaves in place (cosine: half a cycle; cosine_with_restarts: one cycle;
 * polynomial: power 1, lr_end 1e-7); below num_warmup_steps every type but PMGT_LR_CONSTANT returns k / max(1, num_warmup_steps). */
#define PMGT_LR_CONSTANT 0
#define PMGT_LR_CONSTANT_WITH_WARMUP 1
#define PMGT_LR_LINEAR 2
#define PMGT_LR_COSINE 3
#define PMGT_LR_COSINE_WITH_RESTARTS 4
#define PMGT_LR_POLYNOMIAL 5
typedef struct pmgt_lr_schedule {
    int type; /* PMGT_LR_* */
    int64_t num_warmup_steps, num_training_steps;
} pmgt_lr_schedule;
/* pmgt_optimizer_step with the schedule; the weight decay uses lr_t too.  a->step is the schedule's position as well as Adam's.
 * a->scalars is device [8] here -- THE scal [8] LAYOUT of this entry, pmgt_optimizer_step_guarded and the pmgt_op_adamw_scheduled /
 * _guarded entries of pmgt_ops.h: [0] clip coefficient, [1] lr_t / bc1, [2] 1 / sqrt(bc2), [3] total gradient norm (pre-clip), [4] lr_t,
 * [5] guarded entries only: 1 when the step was skipped, else 0; [6..7] never touched.  The unguarded entries neither read nor write
 * [5] either.  Refused (-2): a NULL schedule, an unknown
 * type, num_warmup_steps < 0, num_training_steps <= 0 for linear / cosine / cosine_with_restarts / polynomial, polynomial with
 * lr <= 1e-7 or num_training_steps <= num_warmup_steps.  Three launches, as the unscheduled step (norm partials, prepare, AdamW); the
 * per-phase timers do not bracket this entry. */
int pmgt_optimizer_step_scheduled(pmgt_engine* e, const pmgt_tensors* t, const pmgt_adam* a, const pmgt_lr_schedule* sched, void* stream);

/* The guarded step: what a GradScaler gives the reference under --mp-enabled (pmgt/base_trainer.py:312) -- an optimizer step whose
 * gradients hold an Inf or a NaN is skipped -- decided ON THE DEVICE, so it holds inside a captured step, plus device-side counters and
 * an optional per-step log ring.  The step is bad when the global gradient norm is not finite: any Inf / NaN element, and also finite
 * gradients whose sum of squares overflows fp32 (torch.nn.utils.clip_grad_norm_ on fp32 gradients reports the same Inf norm).
 *   counters  device int64 [4], required: [0] attempts, [1] skipped in total, [2] skipped in a row (a good step resets it), [3] reserved
 *   log_f     device fp32 [log_rows][PMGT_STEP_LOG_FLOATS], row = attempt index % log_rows: [0] loss (NaN when `loss` is NULL), [1] pre-clip
 *             gradient norm, [2] clip coefficient (0 on a skipped step), [3] lr_t, [4] flag: 0 applied, 1 skipped, 2 applied although the
 *             norm is not finite (skip_nonfinite = 0); [5..7] not written
 *   log_i     device int64 [log_rows][2]: [0] attempt index (0-based), [1] *a->step after the step
 *   log_rows  0 = no log (both log pointers may be NULL then)
 *   loss      device fp32 scalar the log copies (e.g. pmgt_outputs.loss of the step's last micro-batch), or NULL
 *   skip_nonfinite  1 = skip bad steps; 0 = count and log only, the step is applied whatever the norm (pmgt_optimizer_step's behaviour) */
#define PMGT_STEP_LOG_FLOATS 8
typedef struct pmgt_step_guard {
    int64_t* counters;
    float* log_f;
    int64_t* log_i;
    int64_t log_rows;
    const float* loss;
    int skip_nonfinite;
} pmgt_step_guard;
/* pmgt_optimizer_step_scheduled (sched = NULL: constant a->lr, then pmgt_optimizer_step bit for bit) with the guard; a->scalars as
 * there, [0..4] bit for bit on an applied step.  A skipped step touches no parameter or moment, does NOT advance *a->step (bias
 * corrections and schedule count applied steps), and writes [0] = 0, [3] = the non-finite norm, [4] = the rate it would have used,
 * [1] and [2] not at all.  Refused (-2): what pmgt_optimizer_step_scheduled refuses of a schedule that is given, a NULL guard or
 * counters, log_rows < 0, log_rows > 0 with a NULL log pointer.  The same three launches, no sync, no allocation: capturable.
 * Added without a bump of pmgt_abi_version(): the ABI grew by addition only (one struct, one entry), nothing existing moved. */
int pmgt_optimizer_step_guarded(pmgt_engine* e, const pmgt_tensors* t, const pmgt_adam* a, const pmgt_lr_schedule* sched,
                                const pmgt_step_guard* guard, void* stream);

/* Validation loss and ROC AUC ON THE DEVICE: `_validation_and_test_step` / `_valid_and_test_epoch_end` (pmgt/pmgt/trainer.py:162-195 --
 * sigmoid(logits) and labels collected per batch, the batch loss weighted by its size, sklearn's roc_auc_score over the epoch) without a
 * device-to-host copy per batch.  The caller owns one workspace of pmgt_eval_workspace_bytes(capacity) bytes (16-byte aligned device memory,
 * capacity = prediction slots, 1 .. 2^26) and passes the same `capacity` to every call on it.  Layout, capr = capacity rounded up to 256:
 *   [0, 64)   scalars: [0] fp64 loss accumulator; uint64 [1] twoU, [2] n_pos, [3] n_neg (written by reduce), [4] scores that were NaN
 *             (counted by append), [5] the n of the last reduce, [6..7] reserved
 *   then      keys uint32 [capr], scores fp32 [capr], labels uint8 [capr] in slot order, then scratch of the reduce.
 * The result STAYS in the workspace: the host reads the 64 scalar bytes with one copy and divides,
 *   loss/val = acc / n_targets_total,   val/auc = twoU / (2 n_pos n_neg)
 * (twoU < 2^53 is exact in a double, so that one division is the only rounding).  Every entry is stream-ordered, allocates nothing,
 * never synchronises and keeps no state outside the workspace.  Refused (-2): NULL / misaligned workspace, a capacity outside the range,
 * slots past the capacity (nothing is written then), n outside [1, capacity] for reduce.
 * Added without a bump of pmgt_abi_version(): the ABI grew by addition only (four entries), nothing existing moved. */
#define PMGT_EVAL_HEADER_BYTES 64
/* pmgt/pmgt/trainer.py:162-195: the storage `outputs` of the validation epoch would take; < 0 for a capacity outside 1 .. 2^26 */
int64_t pmgt_eval_workspace_bytes(int64_t capacity);
/* pmgt/pmgt/trainer.py:162-195: start of a validation epoch -- zeroes the scalars (loss accumulator, NaN counter, last result) */
int pmgt_eval_reset(void* workspace, int64_t capacity, void* stream);
/* pmgt/pmgt/trainer.py:162-195, one validation step: score = 1.0f / (1.0f + expf(-logit)) (accurate expf), key and label != 0 of logits /
 * labels [n] (device fp32) go to slots offset .. offset + n; the key is the order-preserving uint32 image of the score with -0.0f folded
 * onto +0.0f; a NaN score gets no key and counts in scalar [4].  loss (device fp32 scalar, or NULL): acc += (double)loss * n_targets, rounded
 * as the host's `loss_sum += loss.item() * len(batch)`.  offset, n, n_targets are host integers (the sampler knows them). */
int pmgt_eval_append(void* workspace, int64_t capacity, const float* logits, const float* labels, const float* loss, int64_t offset,
                     int64_t n, int64_t n_targets, void* stream);
/* pmgt/pmgt/trainer.py:162-195, epoch end: sorts the keys of slots 0 .. n and writes the Mann-Whitney statistic with midranks in exact
 * integers, twoU = sum over tie groups of p (2 neg_below + q) (p / q = positives / negatives of the group, neg_below = negatives in all lower
 * groups), with n_pos and n_neg.  Bit-reproducible, independent of launch geometry; the slot-order arrays are left as they are, so a
 * reduce can be repeated or follow further appends.  One launch of one workgroup up to 4 096 predictions (the size switch: include/pmgt_ops.h
 * exports it), the multi-tile radix path above. */
int pmgt_eval_reduce(void* workspace, int64_t capacity, int64_t n, void* stream);

/* Top-N ranking metrics ON THE DEVICE: nDCG@k, Recall@k and the per-user loss of `NCFTrainerModel._validation_and_test_step` /
 * `validation_epoch_end` (pmgt/ncf/trainer.py:202-254 over get_ndcg / get_recall, pmgt/metrics.py:16-37: one Python iteration, one topk, one
 * .item() and one device-to-host copy per user, then a MultiLabelBinarizer pass per rank position) from rows of candidate scores that stay
 * on the device.  The caller owns one workspace of pmgt_rank_workspace_bytes(max_users, n_k) bytes (16-byte aligned device memory, max_users =
 * user slots, 1 .. 2^22) and passes the same `max_users` to every call on it; reset comes first.  Limits: a row holds 1 .. PMGT_RANK_MAX_ROW
 * candidates, up to PMGT_RANK_MAX_KS cut-offs `ks`, strictly increasing, each in [1, PMGT_RANK_MAX_K].
 * Per user row, with key = the order-preserving uint32 image of the fp32 score (-0.0f folded onto +0.0f, +-inf at the ends):
 *   rank(p)  = #{c : key(c) > key(p)} + #{c < p : key(c) == key(p)}       -- a permutation of the row; TIES GO TO THE LOWER CANDIDATE
 *              INDEX (torch.topk leaves their order unspecified: this is the project's rule)
 *   hits_k   = #{positives p : rank(p) < k},   recall_k = (double)hits_k / n_pos
 *   dcg_k    = sum of disc[r] over the hit ranks r < k, added in ascending r in fp64,   ndcg_k = dcg_k / idcg[min(n_pos, k) - 1]
 *   loss     = mean over the live candidates of max(x, 0) - x y + log1pf(expf(-|x|)), y = (label != 0) ? 1 : 0, fp32 (BCEWithLogitsLoss
 *              of the row; a label other than 0 or 1 counts as 1)
 * disc[r] = 1 / log2(r + 2) and idcg = cumsum(disc) are the HOST's fp64 tables, handed to reset: the device evaluates no logarithm, and
 * with the ascending adds and one IEEE division the per-user values equal get_ndcg / get_recall called per user, bit for bit.
 * Layout, capr = max_users rounded up to 64:
 *   [0, 128)  written by reduce: fp64 [0..3] sum of ndcg per k, [4..7] sum of recall per k, [8] sum of the losses; uint64 [9] n_users,
 *             [10] users with a NaN logit among their live candidates, [11] users without a positive, [12] slots below n_users that
 *             no append has written since the reset (their records are zeros); [13..15] reserved
 *   then      48 bytes of settings, disc and idcg fp64 [1024] each, and the user records in slot order: ndcg fp64 [n_k][capr],
 *             recall fp64 [n_k][capr], loss fp32 [capr], n_pos int32 [capr], flags uint32 [capr] (bit 0 NaN, bit 1 no positive, bit 2 never
 *             written: reset leaves every record zero with bit 2 set).
 * The result STAYS in the workspace: the host reads the 128 header bytes with one copy and divides by n_users.  Every entry is
 * stream-ordered, allocates nothing, never synchronises, uses no floating-point atomic and keeps no state outside the workspace: the
 * sums do not depend on launch geometry or on how the users were split over appends, and are bitwise repeatable.
 * Refused (-2), writing nothing: a NULL or misaligned pointer, max_users outside its range, row_stride outside [1, PMGT_RANK_MAX_ROW],
 * ks not strictly increasing / outside [1, PMGT_RANK_MAX_K] / more than PMGT_RANK_MAX_KS, user slots past max_users, n_users outside
 * [1, max_users] for reduce.  An append or reduce on a workspace whose last reset was for another max_users (or never ran) writes nothing.
 * Added without a bump of pmgt_abi_version(): the ABI grew by addition only (four entries), nothing existing moved. */
#define PMGT_RANK_HEADER_BYTES 128
#define PMGT_RANK_MAX_ROW 4096
#define PMGT_RANK_MAX_K 1024
#define PMGT_RANK_MAX_KS 4
/* pmgt/ncf/trainer.py:202-254: the storage the per-user results of a ranking evaluation take; < 0 for arguments outside the limits */
int64_t pmgt_rank_workspace_bytes(int64_t max_users, int n_k);
/* pmgt/ncf/trainer.py:202-254, start of an evaluation: zeroes the header and the records (marking every slot as not written), records
 * ks [n_k] and uploads the tables.  ks, disc and idcg are
 * HOST arrays (disc, idcg: fp64 [ks[n_k - 1]], 8-byte aligned); they travel in kernel arguments, so they may be freed when the call returns */
int pmgt_rank_reset(void* workspace, int64_t max_users, const int* ks, int n_k, const double* disc, const double* idcg, void* stream);
/* pmgt/ncf/trainer.py:202-219, one batch of users: logits and labels are device fp32 [n_users][row_stride] (a candidate is positive iff its
 * label != 0), counts device int32 [n_users] = live candidates per row, 1 .. row_stride (entries past the count are padding and are never
 * read; NULL = full rows).  The record of row i goes to slot user_offset + i (a host integer).  One launch, one workgroup per row. */
int pmgt_rank_append(void* workspace, int64_t max_users, const float* logits, const float* labels, const int32_t* counts, int64_t row_stride,
                     int64_t user_offset, int64_t n_users, void* stream);
/* pmgt/ncf/trainer.py:227-254, epoch end: sums the records of slots 0 .. n_users in user order with a fixed tree into the header; the
 * records are left as they are, so a reduce can be repeated or follow further appends.  One launch. */
int pmgt_rank_reduce(void* workspace, int64_t max_users, int64_t n_users, void* stream);

/* Recommendation from the WHOLE catalogue ON THE DEVICE: the eval-mode head of PMGT_NCF (pmgt/pmgt_ncf/models.py:91-105; dropout is the
 * identity) for a batch of users against every item, fused so that nothing per (user, item) pair touches memory except one fp32 logit,
 * and the selection of each user's k best items that the user has not interacted with.  The reference has no such path: its test step
 * (pmgt/ncf/trainer.py:202-219) does `pred.topk(100)` on one sampled candidate list per user.
 *
 * SCORING.  With d = factor_num * 2^(num_layers - 1) the width of the user and item embeddings, layer 0 of the head is linear in the
 * concatenation [user ; item]: W0 = [W0u | W0e] (mlp_layers[0].linear.weight [d][2 d], its first d columns and its last d).  The CALLER
 * computes, once,
 *   pu = mlp_user_embeddings.weight[users] W0u^T         [n][d]
 *   pi = item_table W0e^T + mlp_layers[0].linear.bias    [n_items][d]
 * (two dense products over the item table [n_items][d] and the gathered user rows; plumbing) and the entry computes per pair (r, j)
 *   h1 = relu(pu[r] + pi[j]),   h(i+1) = relu(W_i h_i + b_i) for i = 1 .. num_layers - 1,
 *   scores[r][j] = predict_weight . [gmf_user[users[r]] * gmf_item[j] ; h_L] + predict_bias        (PMGT_NCF_NEUMF_END)
 *   scores[r][j] = predict_weight . h_L + predict_bias                                              (PMGT_NCF_MLP)
 * in fp32 end to end on the exact f32-input matrix instruction (no bf16 anywhere); a NaN in pu or pi reaches the scores (the ReLU keeps
 * it).  Entries [r][n_items .. row_stride) are not written.  All pointers are device memory, the parameters in their state_dict
 * layout (weight[i] = mlp_layers[i].linear.weight [d >> i][d >> (i - 1)] row-major; weight[0] / bias[0] are not read).
 * Covered: factor_num 8, 16, 32 or 64, num_layers 1 .. PMGT_NCF_MAX_LAYERS, d <= 256, both kinds, 1 <= n <= PMGT_NCF_MAX_USERS per call,
 * 1 <= n_items <= 2^31 - 2, row_stride >= n_items.  Refused (-2) before anything is launched, writing nothing: a head outside these
 * limits, a NULL or misaligned buffer, NeuMF-end without its GMF tables, more workgroups than a grid holds.  A user id outside
 * [0, user_num) (NeuMF-end reads the GMF table by it) is never dereferenced: its row of scores is NaN.
 *
 * SELECTION.  Per row of scores [n][row_stride] (n_items live entries; the rest is never read) the k best eligible items in the order of
 * the pmgt_rank entries: key = the order-preserving uint32 image of the fp32 score (-0.0f folded onto +0.0f, a NaN above +inf), descending,
 * and AMONG EQUAL KEYS THE LOWER ITEM INDEX FIRST.  Item j is excluded for row r iff it occurs in the list of users[r] in a device CSR
 * over user ids, indptr int64 [user_num + 1] and excluded int32 [n_excluded] (duplicates are harmless; the CALLER validates the CSR on
 * the host: indptr non-decreasing from 0 to n_excluded, items in [0, n_items); entries outside are skipped, never dereferenced);
 * indptr = NULL: every item is eligible and users is not read.  Output per row: out_items int32 [n][k] and out_scores fp32 [n][k] (the
 * scores as they came in, bit for bit); slots past the eligible count hold item -1 and score -inf; out_flags uint32 [n]:
 * PMGT_TOPK_FLAG_NAN = a NaN among the eligible scores, PMGT_TOPK_FLAG_SHORT = fewer than k eligible items.  The workspace (the caller's,
 * 16-byte aligned, the byte count below for this n and n_items) holds the key image of the rows.  One launch, stream-ordered, no
 * allocation, no wait; integer counting only, so the result is a pure function of the inputs and bitwise repeatable.
 * Refused (-2), writing nothing: k outside [1, PMGT_TOPK_MAX_K], n_items outside [1, 2^31 - 2], n < 1, row_stride < n_items, a NULL or
 * misaligned buffer, a CSR without users / user_num / its item array.
 * Added without a bump of pmgt_abi_version(): the ABI grew by addition only (one struct, three entries), nothing existing moved. */
#define PMGT_NCF_MLP 0
#define PMGT_NCF_NEUMF_END 1
#define PMGT_NCF_MAX_LAYERS 4
#define PMGT_NCF_MAX_USERS 1048576
#define PMGT_TOPK_MAX_K 1024
#define PMGT_TOPK_FLAG_NAN 1u
#define PMGT_TOPK_FLAG_SHORT 2u
typedef struct pmgt_ncf_head {
    int factor_num, num_layers;
    int kind;                                     /* PMGT_NCF_* */
    int reserved;
    const float* weight[PMGT_NCF_MAX_LAYERS];     /* mlp_layers[i].linear.weight; [0] is the caller's (the split layer) */
    const float* bias[PMGT_NCF_MAX_LAYERS];       /* mlp_layers[i].linear.bias */
    const float* predict_weight;                  /* predict_layer.weight [factor_num], NeuMF-end [2 factor_num] = [gmf | mlp] */
    const float* predict_bias;                    /* predict_layer.bias [1] */
    const float* gmf_user;                        /* NeuMF-end: gmf_user_embeddings.weight [user_num][factor_num]; else NULL */
    const float* gmf_item;                        /* NeuMF-end: gmf_item_embeddings.weight [n_items][factor_num]; else NULL */
    int64_t user_num;                             /* rows of gmf_user */
} pmgt_ncf_head;
/* pmgt/pmgt_ncf/models.py:91-105 for n users x n_items items: users int64 [n], scores fp32 [n][row_stride] */
int pmgt_ncf_score(const pmgt_ncf_head* head, const float* pu, const float* pi, const int64_t* users, int64_t n, int64_t n_items,
                   float* scores, int64_t row_stride, void* stream);
/* pmgt/ncf/trainer.py:202-219: the bytes of the key image of n rows of n_items entries; < 0 for arguments outside the limits */
int64_t pmgt_topk_workspace_bytes(int64_t n, int64_t n_items);
/* pmgt/ncf/trainer.py:202-219 (`pred.topk`) for whole rows with the users' known items left out */
int pmgt_topk_rows(const float* scores, int64_t row_stride, int64_t n, int64_t n_items, int k, const int64_t* users, const int64_t* indptr,
                   const int32_t* excluded, int64_t user_num, int64_t n_excluded, void* workspace, int32_t* out_items, float* out_scores,
                   uint32_t* out_flags, void* stream);

/* EVALUATION ON THE WHOLE CATALOGUE ON THE DEVICE: the exact rank of every held-out (user, item) pair among the user's eligible items, and
 * nDCG@k / Recall@k / HR@k / MRR from those ranks.  The reference evaluates on sampled candidate lists (pmgt/ncf/trainer.py:202-254); these
 * entries apply its get_ndcg / get_recall (pmgt/metrics.py:16-37) to each user's whole-catalogue list without building that list.
 *
 * RANKS.  scores fp32 [n][row_stride] (n_items live entries; the rest is never read), users int64 [n], the exclusion CSR exactly as
 * pmgt_topk_rows takes it (indptr = NULL: every item is eligible), and a held-out CSR over the same user ids: held_indptr int64
 * [user_num + 1], held_items int32 [n_heldout] (the CALLER validates both on the host; entries outside are skipped, never dereferenced).
 * With the composite c(j) = key(j) << 32 | (0xFFFFFFFF - j) of the selection above (a NaN score has key 0xFFFFFFFF), for row r of user
 * u = users[r] and every held-out item p of u, at its place in the held-out CSR,
 *   ranks[h] = 1 + #{ j eligible for u, j != p : c(j) > c(p) }
 * = the 1-based place of p in pmgt_topk_rows' order with k = everything; the user's other held-out items count like any item.  A held-out
 * item that is also excluded gets rank 0 and sets PMGT_RANK_HELDOUT_FLAG_EXCLUDED in out_flags[r]; a NaN among the row's eligible scores
 * sets PMGT_TOPK_FLAG_NAN; out_flags uint32 [n] holds no other bit.  A ROW WHOSE USER HAS NO HELD-OUT ITEM (or an id outside
 * [0, user_num)) WRITES NOTHING, its flag word included.  Duplicates in an exclusion list are harmless, AT A COST THAT DEPENDS ON ITS ORDER: a
 * list of L entries in non-decreasing item order (what the Python surface builds) is walked once, L reads per chunk of held-out items; a
 * list in any other order is still right, but every entry is compared with all entries before it, L^2 / 2 reads by the row's one
 * workgroup per chunk -- sort long lists (tens of thousands of entries) before passing them.  A duplicate in a held-out list
 * gets its item's rank at both places; a user in several rows is written by each of them.  One launch, one workgroup per row, no
 * workspace: the row is read from memory once per chunk of PMGT_RANK_HELDOUT_CHUNK held-out items (more are handled by looping); integer
 * counting only, so the result is a pure function of the inputs and bitwise repeatable.
 * Refused (-2), writing nothing: n_items outside [1, 2^31 - 2], n < 1, row_stride < n_items, a NULL or misaligned buffer, user_num < 1,
 * n_heldout < 0 or without its item array, an exclusion CSR without its item array.
 *
 * METRICS.  For the n_users evaluated users (device int64, ids in [0, user_num)) with n_pos = the length of the user's held-out list and
 * the ranks above, per cut-off k of ks (host ints, 1 .. PMGT_RANK_MAX_KS strictly increasing values in [1, PMGT_RANK_MAX_K]):
 *   recall_k = #{rank <= k} / n_pos,   dcg_k = the discounts disc[rank - 1] of the ranks <= k added in ascending rank in fp64,
 *   ndcg_k = dcg_k / idcg[min(n_pos, k) - 1],   hit_k = (min rank <= k),   rr = 1 / min rank
 * (rank 0 is no rank: it hits nothing; a user without a rank has rr = 0 and every record 0).  disc and idcg are DEVICE fp64 [ks[n_k - 1]]:
 * the caller's tables 1 / log2(r + 2) and their running sum -- the device evaluates no logarithm.  records fp64 [3 n_k + 1][n_users]:
 * rows ndcg_k .., recall_k .., hit_k .., rr.  header: 16 words of 8 bytes, fp64 [0 .. 3] the sums of ndcg per k, [4 .. 7] of recall,
 * [8 .. 11] of hit, [12] of rr over the users in a fixed order (thread t of 256 adds the users t, t + 256, .. ascending, then a fixed
 * tree), uint64 [13] n_users, [14] the users whose word of `flags` (uint32 [n_users], aligned with users; NULL: none) has
 * PMGT_TOPK_FLAG_NAN, [15] those with PMGT_RANK_HELDOUT_FLAG_EXCLUDED.  Two launches, no atomic: the same inputs give the same bits.
 * Refused (-2), writing nothing: a NULL or misaligned buffer (flags may be NULL), n_users < 1, user_num < 1, n_heldout < 1, ks outside
 * those limits.
 * Added without a bump of pmgt_abi_version(): two entries, nothing existing moved. */
#define PMGT_RANK_HELDOUT_CHUNK 1024
#define PMGT_RANK_HELDOUT_FLAG_EXCLUDED 4u
#define PMGT_RANK_HELDOUT_HEADER_BYTES 128
int pmgt_rank_heldout(const float* scores, int64_t row_stride, int64_t n, int64_t n_items, const int64_t* users, const int64_t* indptr,
                      const int32_t* excluded, int64_t user_num, int64_t n_excluded, const int64_t* held_indptr, const int32_t* held_items,
                      int64_t n_heldout, int32_t* ranks, uint32_t* out_flags, void* stream);
int pmgt_rank_heldout_reduce(const int32_t* ranks, const int64_t* held_indptr, const int64_t* users, const uint32_t* flags, int64_t n_users,
                             int64_t user_num, int64_t n_heldout, const int* ks, int n_k, const double* disc, const double* idcg,
                             double* records, void* header, void* stream);

/* THE ITEM GRAPH FROM INTERACTIONS ON THE DEVICE (notebooks/PMGT.ipynb cell 20, "Construct Product Graph": C = A A^T over the binary
 * item-by-user matrix, an edge wherever an off-diagonal C[i][j] >= min_count).  The caller passes the two CSR images of the DEDUPLICATED
 * (user, item) pairs, all device memory: item_ptr int64 [num_item + 1] / item_users int32 [n_pairs] (compact user indices in [0, n_users),
 * any order inside a row) and user_ptr int64 [n_users + 1] / user_items int32 [n_pairs], and work int64 [num_item]: work[i] = the sum over
 * the users of item i of the number of items of that user (the length of the row's expansion; it only chooses the row's schedule and must
 * not be below the truth).  Indices outside their ranges are skipped, never dereferenced.
 *   pmgt_item_graph_count  deg_flags uint32 [num_item]: bits 0 .. 30 = the number of j != i with C[i][j] >= min_count, bit 31 = the row did
 *                          not fit the LDS table and was counted by the dense fallback; *max_count (one uint32, ZERO on entry) = the
 *                          largest off-diagonal count seen, by integer atomicMax.
 *   pmgt_item_graph_fill   with row_ptr int64 [num_item + 1] the caller's exclusive scan of those degrees, total = row_ptr[num_item] and
 *                          node_of_item int32 [num_item]: for every row its qualifying neighbours in ASCENDING item order at
 *                          [row_ptr[i], row_ptr[i + 1]): indices = node_of_item[j], counts = C[i][j].  deg_flags is the count pass's, read.
 * slots: the entries of one wave's hash table, a power of two in [PMGT_ITEM_GRAPH_MIN_SLOTS, PMGT_ITEM_GRAPH_MAX_SLOTS]
 * (pmgt_item_graph_default_slots() is the library's choice); a table is filled to 3/4 at most: a row with work <= 3/4 slots is taken by
 * one wave, a longer one by a workgroup with 4 slots entries, and a row with MORE THAN 3 slots DISTINCT NEIGHBOURS by the fallback -- the
 * flag depends on the row alone.
 * scratch: uint32 [scratch_rows][num_item rounded up to a multiple of 4], 16-byte aligned, ZERO on entry and zero again on return; one
 * fallback workgroup per scratch row, 1 <= scratch_rows <= 65535.  Two launches an entry, integer arithmetic only, no sync, no
 * allocation; counts are sums and the stored order comes from a sort: the same inputs give the same bits.
 * Refused (-2) before anything is launched: num_item outside [1, 2^31 - 2], n_pairs outside [1, 2^31 - 1], n_users outside [1, n_pairs],
 * min_count outside [1, 2^31 - 1], slots outside those limits, scratch_rows outside its limits, a NULL or misaligned buffer, total < 1.
 * Added without a bump of pmgt_abi_version(): three entries, nothing existing moved. */
#define PMGT_ITEM_GRAPH_MIN_SLOTS 16
#define PMGT_ITEM_GRAPH_MAX_SLOTS 1024
#define PMGT_ITEM_GRAPH_DEFAULT_SLOTS 1024
int pmgt_item_graph_default_slots(void);
int pmgt_item_graph_count(const int64_t* item_ptr, const int32_t* item_users, const int64_t* user_ptr, const int32_t* user_items,
                          const int64_t* work, int64_t num_item, int64_t n_users, int64_t n_pairs, int64_t min_count, int slots,
                          uint32_t* deg_flags, uint32_t* max_count, uint32_t* scratch, int64_t scratch_rows, void* stream);
int pmgt_item_graph_fill(const int64_t* item_ptr, const int32_t* item_users, const int64_t* user_ptr, const int32_t* user_items,
                         const int64_t* work, int64_t num_item, int64_t n_users, int64_t n_pairs, int64_t min_count, int slots,
                         const uint32_t* deg_flags, const int64_t* row_ptr, const int32_t* node_of_item, int64_t total, int32_t* indices,
                         int32_t* counts, uint32_t* scratch, int64_t scratch_rows, void* stream);

/* NEAREST ITEMS FROM THE EMBEDDINGS ON THE DEVICE: the score of every (query item, catalogue item) pair from ONE table [n_items][d] of fp32
 * rows (the encoder's CLS vectors), as their dot product or their cosine -- what the graph-structure objective scores a pair of nodes by
 * (pmgt/pmgt/losses.py PMGTGraphConstructLoss: F.normalize, then a dot product).  The reference has no such path.  The rows of scores are
 * what pmgt_topk_rows and pmgt_rank_heldout take, with the query items in the place of the users.
 *
 * NORMS.  inv_norm[j] = 1 / max(sqrt(sum_k table[j][k]^2), eps) in fp32, the clamp of F.normalize (its default eps is 1e-12), the sum in ONE
 * fixed order: the fmaf chain over k = 0 .. d - 1 in ascending order from 0, which is dot(j, j) below bit for bit, so that the rounding of
 * the long sum cancels between a dot product and the norms where two rows are alike and s(j, j) is 1 to a few roundings.  One thread a
 * row, 64 rows a wave.  A row with a NaN gets a NaN.  One launch, no atomic.
 *
 * SCORES.  scores[r][j] = s(queries[r], j) for every r in [0, n) and j in [0, n_items), fp32 row-major with row_stride floats a row
 * (entries [r][n_items .. row_stride) are not written; offsets are 64-bit).  dot(i, j) = the fp32 fmaf chain over k = 0 .. d - 1 in ascending
 * order from 0, on the exact f32-input matrix instruction;
 *   inv_norm = NULL (metric "dot"):   s = dot(i, j)
 *   else (metric "cosine"):           s = (dot(i, j) * inv_norm[min(i, j)]) * inv_norm[max(i, j)], each product rounded to fp32.
 * So s(i, j) and s(j, i) have THE SAME BITS, the bits of s(i, j) depend on rows i and j alone -- not on n, the order of the queries or how
 * the catalogue is cut into calls --, and a NaN in row j reaches exactly the scores of row j and column j.  The table is read in place: the
 * query rows are gathered through `queries`, nothing is copied or normalised.  A query id outside [0, n_items) is never dereferenced:
 * its row of scores is NaN.  One launch, stream-ordered, no allocation, no wait, no atomic: the same inputs give the same bits.
 * Covered: 1 <= d <= PMGT_ITEM_SIM_MAX_D, 1 <= n_items <= 2^31 - 2, 1 <= n <= PMGT_NCF_MAX_USERS per call, row_stride >= n_items.  Refused
 * (-2) before anything is launched, writing nothing: a size outside these limits, an eps that is not a positive finite number, a NULL or
 * misaligned buffer (inv_norm may be NULL), more workgroups than a grid holds.
 * Added without a bump of pmgt_abi_version(): two entries, nothing existing moved. */
#define PMGT_ITEM_SIM_MAX_D 1024
int pmgt_item_sim_norms(const float* table, int64_t n_items, int d, float eps, float* inv_norm, void* stream);
int pmgt_item_sim_score(const float* table, const float* inv_norm, const int64_t* queries, int64_t n, int64_t n_items, int d, float* scores,
                        int64_t row_stride, void* stream);

/* RECOMMENDING FROM A USER'S HISTORY ON THE DEVICE (item-kNN): scores[r][j] = agg over i in H(users[r]) of s(i, j) for every r in [0, n) and
 * j in [0, n_items), where s is pmgt_item_sim_score's score over the same table and inv_norm (NULL: metric "dot") and H(u) is the list
 * hist_items[hist_ptr[u] .. hist_ptr[u + 1]) of a CSR over user ids (hist_ptr int64 [user_num + 1], hist_items int32: item ids, every
 * list ASCENDING WITHOUT DUPLICATES; THE CALLER CHECKS the CSR, it is read as it is).  A user the trained heads never saw is served
 * by this, and so is an encoder that has no head yet.  The rows of scores are what pmgt_topk_rows and pmgt_rank_heldout take.
 * One kernel: pmgt_item_sim_score's tile with a segmented reduction over the history rows in its epilogue; the [sum of |H|, n_items] block
 * of item scores is never written, the output is [n][row_stride] fp32 (entries [r][n_items .. row_stride) are not written; offsets are 64-bit).
 *
 * THE SCORE.  s(i, j) has the bits of pmgt_item_sim_score.  With i_0 < i_1 < .. the items of the list in its order:
 *   PMGT_HISTORY_MEAN:  acc = s(i_0, j); acc = acc + s(i_t, j) for t = 1 .. len - 1, every sum rounded to fp32, none contracted;
 *                       score = acc / (float)len, one IEEE division
 *   PMGT_HISTORY_MAX:   the largest s(i_t, j); NaN if any term is NaN; a zero result is +0.0f (the fold of the selection's key)
 * The bits of scores[r][j] depend on H(users[r]), the rows of its items and row j alone -- not on n, the slot r, the other users of the call
 * or how the catalogue is cut into calls: a workgroup owns whole users, and one thread folds a (user, candidate) pair from the first item
 * of the list to the last however long the list is.  A NaN in item row x reaches column x and every score of the users whose list holds
 * x, and nothing else.  A user id outside [0, user_num) or a user with an empty list is never dereferenced: its row of scores is NaN.  An
 * item id outside [0, n_items) in a list is never dereferenced: its terms are NaN.
 * One launch, stream-ordered, no allocation, no wait, no atomic: the same inputs give the same bits.
 * Covered: 1 <= d <= PMGT_ITEM_SIM_MAX_D, 1 <= n_items <= 2^31 - 2, 1 <= n <= PMGT_NCF_MAX_USERS per call, user_num >= 1, lists of any
 * length, row_stride >= n_items.  Refused (-2) before anything is launched, writing nothing: a size outside these limits, an unknown agg, a
 * NULL or misaligned buffer (inv_norm may be NULL; hist_ptr and users: 8 bytes, the rest: 4), more workgroups than a grid holds.
 * Added without a bump of pmgt_abi_version(): one entry, nothing existing moved. */
#define PMGT_HISTORY_MEAN 0
#define PMGT_HISTORY_MAX 1
int pmgt_history_score(const float* table, const float* inv_norm, const int64_t* hist_ptr, const int32_t* hist_items, const int64_t* users,
                       int64_t n, int64_t user_num, int64_t n_items, int d, int agg, float* scores, int64_t row_stride, void* stream);

/* TRUNCATED, WEIGHTED ITEM-kNN ON THE DEVICE over a precomputed neighbour index: the classic item-kNN keeps, per item, only its m most
 * similar items and scores a candidate by the sum over the history items that LIST it.  The index is nbr int32 [n_items][idx_stride] and
 * sim fp32 [n_items][idx_stride], of which the first m columns of every row are used (m <= idx_stride: the index of a smaller m is a prefix
 * of the index of a larger one, so a sweep over m reads one index).  A slot holds a neighbour id or, from the first unused slot of a
 * short row on, -1; THE LIVE IDS OF A ROW ARE PAIRWISE DISTINCT -- THE CALLER CHECKS the index, it is read as it is, and the kernel's
 * freedom from races rests on this.  H(u) is the list hist_items[hist_ptr[u] .. hist_ptr[u + 1]) of pmgt_history_score's CSR (every list
 * ASCENDING WITHOUT DUPLICATES, checked by the caller), hist_weights fp32 aligned with hist_items (ratings, a time decay) or NULL: every
 * weight 1.  The rows of scores are what pmgt_topk_rows and pmgt_rank_heldout take; the output is [n][row_stride] fp32 (entries
 * [r][n_items .. row_stride) and the rows from n on are not written; offsets are 64-bit).  Nothing of the embedding table is read: a user
 * costs |H| m gathered entries and the n_items floats of the row, whatever d was.
 *
 * THE SCORE.  With i_0 < i_1 < .. the items of the list in its order and w_t the weight of entry t, for every r in [0, n), j in [0, n_items):
 *   acc = +0.0f
 *   for t = 0 .. len - 1, in this order:  if j is in the first m slots of row i_t, at slot c:
 *       term = sim[i_t][c]  (hist_weights NULL)   |   w_t * sim[i_t][c] rounded once to fp32
 *       acc  = acc + term   rounded to fp32, never contracted into an fma
 *   scores[r][j] = acc
 * An item that no history item lists scores +0.0f, the empty sum, and a zero result is always +0.0f.  The bits of scores[r][j] depend on
 * H(users[r]), its weights and the index rows of its items alone -- not on n, the slot r, the other users of the call, how the catalogue is
 * cut into tiles or the launch geometry: a workgroup keeps the accumulators of one slot and pmgt_knn_score_tile() consecutive candidates in
 * LDS, each of its waves owns a fixed share of these columns and walks the whole list itself, first entry to last, with plain LDS reads,
 * adds and writes.  A user id outside [0, user_num) or a user with an empty list is never dereferenced: its row of scores is NaN.  A
 * history item outside [0, n_items) is never dereferenced: it makes the whole row NaN.  A neighbour id < 0 or >= n_items is skipped.
 * One launch, stream-ordered, no allocation, no wait, no atomic of any kind: the same inputs give the same bits.
 * Covered: 1 <= m <= 1024 (PMGT_TOPK_MAX_K, what the selection builds) with m <= idx_stride, 1 <= n_items <= 2^31 - 2, 1 <= n <=
 * PMGT_NCF_MAX_USERS per call, user_num >= 1, lists of any length, row_stride >= n_items.  Refused (-2) before anything is launched, writing
 * nothing: a size outside these limits, a NULL or misaligned buffer (hist_weights may be NULL; hist_ptr and users: 8 bytes, the rest: 4),
 * more workgroups than a grid holds (n times the tiles of the catalogue).
 * Added without a bump of pmgt_abi_version(): two entries, nothing existing moved. */
int pmgt_knn_score_tile(void);      /* the candidates a workgroup owns (KNN_T of ops/knn_score.hip): where the catalogue is cut */
int pmgt_knn_score(const int32_t* nbr, const float* sim, int64_t idx_stride, int m, const int64_t* hist_ptr, const int32_t* hist_items,
                   const float* hist_weights /* may be NULL */, const int64_t* users, int64_t n, int64_t user_num, int64_t n_items,
                   float* scores, int64_t row_stride, void* stream);

/* Training of the head of PMGT_NCF over a FROZEN item table ON THE DEVICE (the reference's downstream step, pmgt/ncf/trainer.py:183-200 with
 * `--item-init-emb-path`: embed_item_MLP frozen, BCEWithLogitsLoss): for n (user, item, label) pairs the mean loss, the logits and the
 * gradient of that loss with respect to EVERY parameter of the head, in two launches, no sync, no allocation, no atomic: capturable, and
 * the same inputs give the same bits.  With d = factor_num * 2^(num_layers - 1):
 *   x0 = [mlp_user[u] ; table[i]],  h(l+1) = relu(W_l h_l + b_l) for l = 0 .. num_layers - 1   (W_0 UNSPLIT, [d][2 d]; dropout is 0),
 *   z = predict_weight . [gmf_user[u] * gmf_item[i] ; h_L] + predict_bias   (PMGT_NCF_MLP: predict_weight . h_L + predict_bias),
 *   loss = mean over the pairs of max(z, 0) - z y + log1p(exp(-|z|)),   dz = (sigmoid(z) - y) / n,   the ReLU passes where h > 0.
 * THE PARAMETERS are ONE flat fp32 buffer, the gradients another of the same layout; pmgt_ncf_train_layout gives the offset in floats of
 * each tensor, in this order of slots (row-major, the state_dict's shapes), -1 for a tensor the head does not have:
 *   [0] mlp_user_embeddings.weight [user_num][d]
 *   [1] gmf_user_embeddings.weight [user_num][factor_num]      [2] gmf_item_embeddings.weight [item_num][factor_num]      (NeuMF-end)
 *   [3 + 2 l] mlp_layers.l.linear.weight [d >> l][2 (d >> l)]    [4 + 2 l] mlp_layers.l.linear.bias [d >> l]
 *   [11] predict_layer.weight [factor_num] or [2 factor_num] = [gmf | mlp]      [12] predict_layer.bias [1]
 * and returns the parameter count; the tensors are packed in slot order, the three embedding tables first.
 * THE GRADIENT BUFFER IS WRITTEN WHOLE: embedding rows no pair touches hold +0.0.  Rows hit by several pairs are summed in pair order,
 * the weight gradients over the pairs in one fixed order (32-pair chunks dealt to four accumulators, added as (0 + 1) + (2 + 3)).
 * users / items int64 [n] (ids inside the tables: THE CALLER CHECKS THEM, they are read as they are), labels fp32 [n], table fp32
 * [item_num][d], loss one device float, logits fp32 [n] or NULL; workspace: pmgt_ncf_train_workspace_bytes(...) bytes of 16-byte aligned
 * device memory.  Covered: the heads pmgt_ncf_score covers (one rule, stated there), 1 <= n <= PMGT_NCF_TRAIN_MAX_PAIRS.
 * Refused (-2; the two sizing entries return it as their value) before anything is launched:
 * a head or n outside these limits, a NULL or misaligned buffer (table, parameters, gradients and workspace: 16 bytes), a short workspace.
 * Added without a bump of pmgt_abi_version(): one struct, three entries, nothing existing moved. */
#define PMGT_NCF_TRAIN_MAX_PAIRS 65536
#define PMGT_NCF_TRAIN_TENSORS 13
typedef struct pmgt_ncf_train {
    int factor_num, num_layers;
    int kind;                                     /* PMGT_NCF_* */
    int reserved;
    int64_t user_num, item_num;                   /* rows of the user tables; rows of `table` and of gmf_item */
    const float* table;                           /* item embeddings [item_num][d]; only read */
    const float* params;                          /* the flat parameters */
    float* grads;                                 /* the flat gradients, written whole */
} pmgt_ncf_train;
int64_t pmgt_ncf_train_layout(int factor_num, int num_layers, int kind, int64_t user_num, int64_t item_num, int64_t* offsets);
int64_t pmgt_ncf_train_workspace_bytes(int factor_num, int num_layers, int kind, int64_t n);
int pmgt_ncf_train_grad(const pmgt_ncf_train* head, const int64_t* users, const int64_t* items, const float* labels, int64_t n, float* loss,
                        float* logits, void* workspace, int64_t workspace_bytes, void* stream);
/* THE ITEM TABLE TRAINED WITH THE HEAD (pmgt/ncf/trainer.py:168-179: embed_item_MLP is initialised from the exported embeddings and keeps
 * requires_grad unless --freeze-item-init-emb is passed; scripts/run_ncf.sh does not pass it).  pmgt_ncf_train_grad_table takes the
 * arguments of pmgt_ncf_train_grad plus table_grad fp32 [item_num][d], 16-byte aligned; it does all that entry does -- loss, logits and
 * the head's gradients have the same bits -- and writes d loss / d table WHOLE: rows no pair touches hold +0.0, rows hit by several
 * pairs are summed in pair order (the rule of gmf_item_embeddings, for both kinds: an MLP head has no GMF rows, only the table's).  The
 * data gradient of layer 0 then covers all 2 d columns of W_0, one row [2 d] per pair in the workspace, which is larger by n d floats:
 * pmgt_ncf_train_table_workspace_bytes.  Still two launches, no atomic, no sync, no allocation; `table` is only read, so `table` and
 * table_grad may lie behind the head in the caller's flat parameter and gradient buffers (one optimizer call then steps both).  Refused
 * (-2) before anything is launched: what pmgt_ncf_train_grad refuses, a NULL or misaligned table_grad, a workspace below that size.
 * Added without a bump of pmgt_abi_version(): two entries, nothing existing moved. */
int64_t pmgt_ncf_train_table_workspace_bytes(int factor_num, int num_layers, int kind, int64_t n);
int pmgt_ncf_train_grad_table(const pmgt_ncf_train* head, const int64_t* users, const int64_t* items, const float* labels, int64_t n,
                              float* loss, float* logits, float* table_grad, void* workspace, int64_t workspace_bytes, void* stream);
/* THE HEAD TRAINED WITH DROPOUT (PMGT_NCF.head in training mode: a Dropout behind every Linear, emb_dropout on the concatenated
 * [user ; item] input and on the GMF product; every config/hpo/hpo_ncf_*_params.yaml searches both p over [0, 0.8]).  With m = 0 or
 * 1 / (1 - p), drawn per element:
 *   x0 = m_e [mlp_user[u] ; table[i]],   h(l+1) = relu(m_l (W_l h_l + b_l)),   NeuMF-end: g = m_g (gmf_user[u] * gmf_item[i]),
 * m_e and m_g at p_emb (two masks of their own), m_l at p_layer[l]; everything else as pmgt_ncf_train_grad states it, and the gradients are
 * those of this function: d x0 carries m_e down to the embedding rows (and to table_grad), the ReLU passes where the DROPPED activation is
 * > 0 with the factor 1 / (1 - p_l).  THE MASKS come from the engine's counter-based RNG (make_drop_key / drop_keep4: one hash pair
 * decides 4 neighbouring columns, an element is kept when its 16-bit lane >= thr >> 16, thr = (uint32)(p 2^32); the scale is the fp32
 * value 1 / (1 - p)) over `rng`, a device {seed, step} pair of the caller's own, read by the kernels: a captured call replays with fresh
 * masks when an earlier kernel advances the step (pmgt_op_adamw does).  A site's ROW is the pair's index within the call, its COLUMN the
 * feature; the SITE IDS (constants of ops/ncf_head.h, mirrored in _lib.py), distinct from each other (the pair is the caller's, so they
 * need not avoid the engine's):
 *   NCF_SITE_EMB   64       [n][2 d], the user half first
 *   NCF_SITE_GMF   65       [n][factor_num]
 *   NCF_SITE_LAYER 72 + l   [n][d >> l], the output of layer l
 * so the test entry pmgt_op_dropout_keep with (rng, p, site, n, cols) writes exactly the decisions a call draws, and the call is a pure function of
 * (inputs, seed, step).  table_grad NULL: the table is frozen (pmgt_ncf_train_grad's outputs and workspace); else it is trained
 * (pmgt_ncf_train_grad_table's).  Still two launches, no atomic, no sync, no allocation, the gradient buffers written whole, the same
 * workspace sizes.  With every p equal to 0 the call runs the kernels of the two entries above: the same bits, `rng` not read.
 * Refused (-2) before anything is launched: what those entries refuse, a NULL drop, a p_emb or p_layer[l < num_layers] that is NaN or
 * outside [0, 1), and any p > 0 with a NULL or 8-byte-misaligned rng.
 * Added without a bump of pmgt_abi_version(): one struct, one entry, nothing existing moved. */
typedef struct pmgt_ncf_dropout {
    const uint64_t* rng;                          /* device {seed, step}; read only when a p is > 0 */
    float p_emb;                                  /* emb_dropout.p: the input of layer 0 and the GMF product */
    float p_layer[PMGT_NCF_MAX_LAYERS];           /* mlp_layers[l].dropout.p */
} pmgt_ncf_dropout;
int pmgt_ncf_train_grad_dropout(const pmgt_ncf_train* head, const int64_t* users, const int64_t* items, const float* labels, int64_t n,
                                float* loss, float* logits, float* table_grad /* NULL: frozen table */, const pmgt_ncf_dropout* drop,
                                void* workspace, int64_t workspace_bytes, void* stream);
/* THE HEAD ON PER-PAIR ITEM ROWS (fine-tuning the encoder through the head, pmgt/pmgt_ncf/models.py:77-105: every pair has a sampled context
 * of its own, so its item embedding is the CLS state of THAT context and no row of a table).  The function is the dropout entry's above
 * (drop NULL: no dropout) with one difference: the item half of layer 0's input of pair p is row p of x_item, fp32 [n][d], contiguous, 16-byte
 * aligned, where the other entries read table[items[p]].  `items` still addresses gmf_item_embeddings (NeuMF-end); head->table is NOT READ
 * (it may be NULL) and head->item_num is the row count of gmf_item.  Written: everything the table entry writes but the table's gradient
 * (loss, logits, the head's gradient buffer whole, with the same bits as that entry's when x_item[p] = table[items[p]]) and d_item fp32
 * [n][d], 16-byte aligned, whole: row p = d loss / d x_item[p], with dropout under the emb mask exactly as table_grad is.  NOTHING IS SUMMED
 * ACROSS PAIRS: two pairs on one item keep separate rows.  Sites, rows and columns of the masks are unchanged (row = the pair's index).
 * LAUNCHES: TWO, the kernels of the table entry (the second gains one role that copies the item half of the per-pair data gradient out of
 * the workspace); no atomic, no sync, no allocation, capturable, the same bits for the same inputs.  Workspace:
 * pmgt_ncf_train_rows_workspace_bytes (the table entry's size).  Refused (-2) before anything is launched: what the entries above refuse
 * (but the table), a NULL or misaligned x_item or d_item.
 * Added without a bump of the ABI version: two entries, nothing existing moved. */
int64_t pmgt_ncf_train_rows_workspace_bytes(int factor_num, int num_layers, int kind, int64_t n);
int pmgt_ncf_train_grad_rows(const pmgt_ncf_train* head, const int64_t* users, const int64_t* items, const float* labels, int64_t n, float* loss,
                             float* logits, const float* x_item, float* d_item, const pmgt_ncf_dropout* drop /* NULL: none */,
                             void* workspace, int64_t workspace_bytes, void* stream);
/* THE REFERENCE'S STAND-ALONE NCF CLASS (pmgt/ncf/models.py; pmgt_amd/ncf.py restates it): the model owns its four embedding tables,
 * its layer may carry a LayerNorm, and it has two more kinds.  With d = factor_num 2^(num_layers - 1), per pair (u, i):
 *   h_0 = m_e [embed_user_MLP[u] ; embed_item_MLP[i]],   h_(l+1) = relu(LN_l(m_l (W_l h_l + b_l)))      (LN_l absent without use_layer_norm)
 *   g = m_g (embed_user_GMF[u] * embed_item_GMF[i])
 *   z = predict_layer . h_L (MLP),  . g (GMF),  . [g ; h_L] (NeuMF-end; NeuMF-pre is trained exactly as NeuMF-end),  + predict_layer.bias
 * LN is torch.nn.LayerNorm (biased variance, (x - mean) / sqrt(var + eps) gamma + beta); the dropout sits BEFORE it.  The masks, their
 * sites and the RNG are pmgt_ncf_train_grad_dropout's; kind GMF draws the gmf site alone.
 * THE PARAMETERS are ONE flat fp32 buffer holding only what the kind trains, the gradients another of the same layout;
 * pmgt_ncf_model_layout gives the offsets in floats (-1: not trained) in the slot order
 *   0 embed_user_MLP   1 embed_user_GMF   2 embed_item_GMF   3 + 4 l: W_l, b_l, gamma_l, beta_l   19, 20 predict_layer.weight, .bias
 *   21 embed_item_MLP (train_items: behind the rest, its offset rounded up to a multiple of 8 floats)
 * and returns the count.  Without LayerNorm, kinds MLP / NeuMF-end / NeuMF-pre, the layout is pmgt_ncf_train_layout's followed by the table,
 * and the call IS pmgt_ncf_train_grad / _table / _dropout on the same buffers: their bits, their workspace sizes.  Kind GMF reads and
 * trains no MLP tensor (item_table, table_grad and train_items are ignored; d is not limited).
 * m->item_table is embed_item_MLP.weight [item_num][d] and may point into params; with train_items, table_grad [item_num][d] is written
 * whole and may point into grads.  Written: loss (one float), logits (fp32 [n] or NULL), the gradient buffer whole (rows of an embedding
 * table that no pair touches hold +0.0; rows hit by several pairs are summed in pair order).  TWO launches, no atomic, no sync, no
 * allocation, capturable, the same bits for the same inputs.  Workspace: pmgt_ncf_model_workspace_bytes, 16-byte aligned.
 * Refused (-2) before anything is launched: factor_num not 8 / 16 / 32 / 64, num_layers outside [1, 4], d > 256 (not GMF), an unknown
 * kind, a layer_norm_eps that is not finite or negative, n outside [1, PMGT_NCF_TRAIN_MAX_PAIRS], a NULL or misaligned buffer (16 bytes
 * for the float buffers, 8 for the ids and the rng), a short workspace, a p that is NaN or outside [0, 1), any p > 0 without the rng.
 * Added without a bump of pmgt_abi_version(): one struct, three entries, nothing existing moved. */
enum {
    PMGT_NCF_GMF = 2,                             /* the kinds after PMGT_NCF_MLP and PMGT_NCF_NEUMF_END */
    PMGT_NCF_NEUMF_PRE = 3,
    PMGT_NCF_MODEL_TENSORS = 22                   /* the slots of pmgt_ncf_model_layout */
};
typedef struct pmgt_ncf_model {
    int factor_num, num_layers;
    int kind;                                     /* PMGT_NCF_MLP, _NEUMF_END, _GMF, _NEUMF_PRE */
    int use_layer_norm;
    float layer_norm_eps;
    int train_items;                              /* embed_item_MLP is trained: table_grad is written */
    int64_t user_num, item_num;
    const float* item_table;                      /* embed_item_MLP.weight [item_num][d]; only read; may point into params */
    const float* params;                          /* the flat parameters */
    float* grads;                                 /* the flat gradients, written whole */
    float* table_grad;                            /* train_items: [item_num][d], written whole; may point into grads */
} pmgt_ncf_model;
int64_t pmgt_ncf_model_layout(int factor_num, int num_layers, int kind, int use_layer_norm, int train_items, int64_t user_num, int64_t item_num,
                              int64_t* offsets);
int64_t pmgt_ncf_model_workspace_bytes(int factor_num, int num_layers, int kind, int use_layer_norm, int train_items, int64_t n);
int pmgt_ncf_model_train_grad(const pmgt_ncf_model* m, const int64_t* users, const int64_t* items, const float* labels, int64_t n, float* loss,
                              float* logits /* or NULL */, const pmgt_ncf_dropout* drop /* or NULL */, void* workspace, int64_t workspace_bytes,
                              void* stream);
/* THE STAND-ALONE NCF CLASS SCORED AGAINST THE WHOLE CATALOGUE (the eval-mode head of the model above for n users x n_items items; what
 * pmgt_ncf_score is to PMGT_NCF).  With pu and pi the caller's split of layer 0 exactly as pmgt_ncf_score states it (pu = embed_user_MLP[users]
 * W0u^T [n][d], pi = item_table W0e^T + b_0 [n_items][d]), per pair (r, j):
 *   h_1 = relu(LN_0(pu[r] + pi[j])),   h_(l+1) = relu(LN_l(W_l h_l + b_l)) for l = 1 .. num_layers - 1      (LN_l absent without use_layer_norm)
 *   scores[r][j] = predict . h_L (MLP),  . g (GMF),  . [g ; h_L] (NeuMF-end, NeuMF-pre)  + predict_bias,   g = gmf_user[users[r]] * gmf_item[j]
 * LN is the LayerNorm of pmgt_ncf_model_train_grad: two passes (mean, then the squared deviations), biased variance, 1 / sqrt(var + eps).
 * fp32 end to end on the exact f32-input matrix instruction; one float stored per pair; no atomic, the same bits for the same inputs;
 * entries [r][n_items .. row_stride) are not written.  A NaN in a row of pi (or of gmf_item) reaches every score of that item and no other.
 * WITHOUT LayerNorm, kinds MLP / NeuMF-end / NeuMF-pre, the call IS pmgt_ncf_score on the same buffers: its bits.  Kind GMF reads
 * predict_weight [factor_num], the two GMF tables and users only (pu, pi and every layer pointer are ignored, num_layers is not limited).
 * A user id outside [0, user_num) (read by the kinds with a GMF branch) is never dereferenced: its row of scores is NaN.
 * Covered: factor_num 8, 16, 32 or 64; kinds but GMF: num_layers 1 .. PMGT_NCF_MAX_LAYERS and d <= 256; 1 <= n <= PMGT_NCF_MAX_USERS,
 * 1 <= n_items <= 2^31 - 2, row_stride >= n_items.  Refused (-2) before anything is launched, writing nothing: a model outside these
 * limits, an unknown kind, a layer_norm_eps that is not finite or negative, a NULL or misaligned buffer, use_layer_norm without gamma /
 * beta of every layer, a kind with the GMF branch without its tables, more workgroups than a grid holds.
 * Added without a bump of pmgt_abi_version(): one struct, one entry, nothing existing moved. */
typedef struct pmgt_ncf_model_head {
    int factor_num, num_layers;
    int kind;                                     /* PMGT_NCF_MLP, _NEUMF_END, _GMF, _NEUMF_PRE */
    int use_layer_norm;
    float layer_norm_eps;
    int reserved;
    int64_t user_num;                             /* rows of gmf_user */
    const float* weight[PMGT_NCF_MAX_LAYERS];     /* the Linear of layer i [d >> i][d >> (i - 1)]; [0] is the caller's (the split layer) */
    const float* bias[PMGT_NCF_MAX_LAYERS];       /* [0] is the caller's too: it is in pi */
    const float* gamma[PMGT_NCF_MAX_LAYERS];      /* use_layer_norm: the LayerNorm of layer i [d >> i], layer 0 included */
    const float* beta[PMGT_NCF_MAX_LAYERS];
    const float* predict_weight;                  /* predict_layer.weight [factor_num], both branches [2 factor_num] = [gmf | mlp] */
    const float* predict_bias;                    /* predict_layer.bias [1] */
    const float* gmf_user;                        /* embed_user_GMF.weight [user_num][factor_num]; kind MLP: NULL */
    const float* gmf_item;                        /* embed_item_GMF.weight [n_items][factor_num]; kind MLP: NULL */
} pmgt_ncf_model_head;
int pmgt_ncf_model_score(const pmgt_ncf_model_head* head, const float* pu, const float* pi, const int64_t* users, int64_t n, int64_t n_items,
                         float* scores, int64_t row_stride, void* stream);

/* The DEEP & CROSS NETWORK of the reference's click-through experiment ON THE DEVICE (pmgt/dcn/models.py, scripts/run_dcn.sh): for n
 * (user, item, label) pairs the logits (pmgt_dcn_forward) or the mean loss, the logits and the gradient of that loss with respect to
 * EVERY trained parameter, both embedding tables included (pmgt_dcn_train_grad), in two launches, no sync, no allocation, no atomic:
 * capturable, and the same inputs give the same bits.  With E = factor_num * 2^deep_layers, D = 2 E, L = deep_layers, C = cross_layers:
 *   x0 = [user_embeddings[u] ; item_embeddings[i]]                                                   (both dropouts are 0)
 *   cross   x^(0) = x0,  s_c = x^(c) . w_c,  x^(c+1) = LN_c(x0 s_c + x0)   c = 0 .. C - 1   (the layer adds x0, NOT x^(c); the
 *           `bias` of the reference's cross layer is never read and is no part of the buffers)
 *   deep    h_0 = x0,  h_(l+1) = relu(LN_l(W_l h_l + b_l)),  W_l [D >> (l + 1)][D >> l]   l = 0 .. L - 1
 *   z = output_weight . [x^(C) ; h_L] + output_bias,   loss = mean of max(z, 0) - z y + log1p(exp(-|z|)),   dz = (sigmoid(z) - y) / n
 * LN(v) = (v - mean) / sqrt(var + layer_norm_eps) gamma + beta, mean and BIASED variance over the row (torch.nn.LayerNorm); with
 * use_layer_norm = 0 it is the identity and the gamma / beta slots are absent.  The ReLU passes where h > 0.
 * THE PARAMETERS are ONE flat fp32 buffer, the gradients another of the same layout; pmgt_dcn_layout gives the offset in floats of each
 * tensor in this order of PMGT_DCN_TENSORS slots (row-major, the state_dict's shapes; -1 for a tensor the model does not have) and
 * returns the parameter count; the tensors are packed in slot order:
 *   [0] user_embeddings.weight [user_num][E]      [1] item_embeddings.weight [item_num][E]
 *   [2 + 4 l] deep_net.layers.l.linear.weight [D >> (l + 1)][D >> l]   [3 + 4 l] .linear.bias   [4 + 4 l] .layer_norm.weight   [5 + 4 l] .layer_norm.bias
 *   [18 + 3 c] cross_net.layers.c.weight [D]      [19 + 3 c] .layer_norm.weight [D]      [20 + 3 c] .layer_norm.bias [D]
 *   [36] output_layer.weight [D + 2 factor_num] = [cross | deep]      [37] output_layer.bias [1]
 * Every tensor but the last has a multiple of 8 floats.
 * THE GRADIENT BUFFER IS WRITTEN WHOLE: embedding rows no pair touches hold +0.0; rows hit by several pairs are summed in pair order,
 * for both tables.  d x0 of a pair is ((cross layer C - 1's term + ... + layer 0's) + d x^(0)) + the deep net's.  The sums over the
 * pairs have one fixed order: the Linear weights, their biases and the output layer (the loss with them) over 32-pair chunks dealt to
 * four accumulators, added as (0 + 1) + (2 + 3); the column sums (gamma, beta and w_c gradients) over the pairs p = a, a + 4, ... in
 * four accumulators a = 0 .. 3, added the same way.
 * pmgt_dcn_forward writes the logits pmgt_dcn_train_grad writes, bit for bit: the same forward code without the stores of the backward;
 * it reads head->params only (grads may be NULL).
 * users / items int64 [n] (ids inside the tables: THE CALLER CHECKS THEM, they are read as they are), labels fp32 [n], loss one device
 * float, logits fp32 [n] (pmgt_dcn_train_grad: or NULL); workspace: pmgt_dcn_workspace_bytes(...) bytes of 16-byte aligned device memory
 * (one size serves both entries).  Covered: factor_num in {8, 16, 32, 64}, 1 <= L <= PMGT_DCN_MAX_DEEP with E <= 256, 1 <= C <=
 * PMGT_DCN_MAX_CROSS, 1 <= n <= PMGT_DCN_MAX_PAIRS, user_num and item_num in [1, 2^31 - 2].
 * Refused (-2; the layout and sizing entries return it as their value) before anything is launched: a shape or n outside these limits, a
 * NULL or misaligned buffer (parameters, gradients and workspace: 16 bytes), a short workspace, a layer_norm_eps that is NaN or negative.
 * Added without a bump of pmgt_abi_version(): one struct, four entries, nothing existing moved. */
#define PMGT_DCN_MAX_DEEP 4
#define PMGT_DCN_MAX_CROSS 6
#define PMGT_DCN_TENSORS 38
#define PMGT_DCN_MAX_PAIRS 65536
typedef struct pmgt_dcn_head {
    int factor_num, deep_layers, cross_layers, use_layer_norm;
    float layer_norm_eps;
    int reserved;
    int64_t user_num, item_num;                   /* rows of the two embedding tables */
    const float* params;                          /* the flat parameters */
    float* grads;                                 /* the flat gradients, written whole (pmgt_dcn_forward: not read, may be NULL) */
} pmgt_dcn_head;
int64_t pmgt_dcn_layout(int factor_num, int deep_layers, int cross_layers, int use_layer_norm, int64_t user_num, int64_t item_num,
                        int64_t* offsets);
int64_t pmgt_dcn_workspace_bytes(int factor_num, int deep_layers, int cross_layers, int use_layer_norm, int64_t n);
int pmgt_dcn_forward(const pmgt_dcn_head* head, const int64_t* users, const int64_t* items, int64_t n, float* logits, void* workspace,
                     int64_t workspace_bytes, void* stream);
int pmgt_dcn_train_grad(const pmgt_dcn_head* head, const int64_t* users, const int64_t* items, const float* labels, int64_t n,
                        float* loss, float* logits /* or NULL */, void* workspace, int64_t workspace_bytes, void* stream);
/* THE DCN TRAINED WITH DROPOUT (pmgt/dcn/models.py in training mode; scripts/run_dcn.sh passes --emb-dropout 0.2 and both
 * config/hpo/hpo_dcn*_params.yaml search emb_dropout and dropout over [0, 0.8]).  With m = 0 or 1 / (1 - p), drawn per element:
 *   x0 = m_e [user_embeddings[u] ; item_embeddings[i]]                                        m_e at p_emb,      [n][D]
 *   cross   s_c = x^(c) . w_c,  x^(c+1) = LN_c(m_c (x0 s_c) + x0)                             m_c at p_cross[c], [n][D]
 *           (the added x0 is the already dropped x0 and is not masked again)
 *   deep    h_(l+1) = relu(LN_l(m_l (W_l h_l + b_l)))                                         m_l at p_deep[l],  [n][D >> (l + 1)]
 *           (the dropout sits BEFORE the LayerNorm: dropped zeros enter the layer's statistics)
 * the output layer and the loss as pmgt_dcn_train_grad states them, and the gradients are those of this function: dy_l = m_l LNbwd(..)
 * (without LayerNorm the ReLU passes where the DROPPED activation is > 0, with the factor 1 / (1 - p_l)), ds_c = sum_j g_j m_cj x0_j,
 * d x0 += g (m_c s_c) + g, and d x0 carries m_e down to the embedding rows.  A cross layer whose own mask is drawn has a non-zero gradient
 * for w_c, and gamma / beta of cross layer c stop being degenerate when p_cross[c + 1] > 0.  THE MASKS come from the engine's counter-based
 * RNG exactly as pmgt_ncf_train_grad_dropout describes it, over `rng`, a device {seed, step} pair of the caller's own; none is stored: they
 * are drawn again wherever the backward and the second launch need them.  A site's ROW is the pair's index within the call, its COLUMN the
 * feature; the SITE IDS (constants of ops/ncf_head.h, mirrored in _lib.py), distinct from each other:
 *   DCN_SITE_EMB   64       [n][D], the user half first
 *   DCN_SITE_DEEP  72 + l   [n][D >> (l + 1)], the Linear output of deep layer l
 *   DCN_SITE_CROSS 80 + c   [n][D], the product x0 s_c of cross layer c
 * so pmgt_op_dropout_keep with (rng, p, site, n, cols) writes exactly the decisions a call draws, and the call is a pure function of
 * (inputs, seed, step).  Still two launches, no atomic, no sync, no allocation, the gradient buffer written whole, the same workspace size.
 * A site with p = 0 draws nothing; with every p equal to 0 the call runs the kernels of pmgt_dcn_train_grad: the same bits, `rng` not read.
 * Refused (-2) before anything is launched: what pmgt_dcn_train_grad refuses, a NULL drop, a p_emb, p_deep[l < L] or p_cross[c < C] that is
 * NaN or outside [0, 1), and any p > 0 with a NULL or 8-byte-misaligned rng.
 * Added without a bump of pmgt_abi_version(): one struct, one entry, nothing existing moved. */
typedef struct pmgt_dcn_dropout {
    const uint64_t* rng;                          /* device {seed, step}; read only when a p is > 0 */
    float p_emb;                                  /* emb_dropout.p: the concatenated input */
    float p_deep[PMGT_DCN_MAX_DEEP];              /* deep_net.layers[l].dropout.p */
    float p_cross[PMGT_DCN_MAX_CROSS];            /* cross_net.layers[c].dropout.p */
} pmgt_dcn_dropout;
int pmgt_dcn_train_grad_dropout(const pmgt_dcn_head* head, const int64_t* users, const int64_t* items, const float* labels, int64_t n,
                                float* loss, float* logits /* or NULL */, const pmgt_dcn_dropout* drop, void* workspace,
                                int64_t workspace_bytes, void* stream);
/* THE DCN SCORED AGAINST THE WHOLE CATALOGUE (the eval-mode model above for n users x n_items items; what pmgt_ncf_model_score is to the
 * NCF class).  The deep net is the NCF tower with d = E, layers L and last width 2 F: pu = user_embeddings[users] W_0[:, :E]^T [n][E] and
 * pi = item_table W_0[:, E:]^T + b_0 [n_items][E] are the caller's split of deep layer 0, and per pair (r, j)
 *   h_1 = relu(LN_0(pu[r] + pi[j])),   h_(l+1) = relu(LN_l(W_l h_l + b_l)) for l = 1 .. L - 1      (LN_l absent without use_layer_norm)
 * on the exact f32-input matrix instruction (L = 1: a vector kernel, one pair a thread), LN with two passes, biased variance and
 * 1 / sqrt(var + eps).  THE CROSS NET COLLAPSES because its layer adds x0: with w_C := output_weight[:D], the half of a D-vector [0, E) for
 * a user row and [E, D) for an item row, and for a table row v of a half
 *   d_c(v) = sum_j v_j g_c[j],   g_0 = w_0[half],   g_c = w_c[half] (no LayerNorm) or gamma_(c-1)[half] * w_c[half] (LayerNorm),   c = 1 .. C
 *   without LayerNorm   a = 1;  for c = 0 .. C-1: a = a (d_c(u) + d_c(i)) + 1;   z_cross = a (d_C(u) + d_C(i))
 *   with LayerNorm      mu(v) the row mean, q(v) = sum_j (v_j - mu(v))^2,  m0 = (mu(u) + mu(i)) / 2,
 *                       v0 = (q(u) + q(i) + E ((mu(u) - m0)^2 + (mu(i) - m0)^2)) / D;   s = d_0(u) + d_0(i);
 *                       for c = 0 .. C-1: k = s + 1, t = k / sqrt(k^2 v0 + eps), s = t (d_(c+1)(u) + d_(c+1)(i) - m0 K_c) + B_c;   z_cross = s
 *                       K_c = sum_D gamma_c w_(c+1),  B_c = sum_D beta_c w_(c+1)
 *   scores[r][j] = (z_cross + output_weight[D:] . h_L) + output_bias
 * pmgt_dcn_score_rows writes, for `rows` rows of a table [rows][E] of `half` (0: user rows, 1: item rows), PMGT_DCN_SCORE_ROW_STRIDE floats
 * a row: [0] mu, [1] q (both 0 without LayerNorm, never read then), [2 + c] d_c for c = 0 .. C, zeros behind.  One wave a row, a fixed
 * order of sums.  The caller runs it once over the item table and once a call over the gathered user rows user_embeddings[users].
 * pmgt_dcn_score reads those two arrays (user_rows [n][stride], item_rows [n_items][stride]) and, with LayerNorm, consts: K_c at [c] and
 * B_c at [PMGT_DCN_MAX_CROSS + c], 2 PMGT_DCN_MAX_CROSS device floats (without LayerNorm it is not read and may be NULL).  Of head->params
 * it reads the deep layers 1 .. L - 1, every deep LayerNorm, output_weight[D:] and output_bias -- a trainer's flat buffer serves in place;
 * neither embedding table is read (head->item_num only addresses the layout; n_items is the row count of pi and item_rows).
 * fp32 end to end; one float stored per pair; no atomic, the same bits for the same inputs; entries [r][n_items .. row_stride) are not
 * written.  A NaN in an item's row reaches every score of that item and no other, a NaN in a user's row that user's scores only.  A user
 * id outside [0, user_num) is never dereferenced: its row of scores is NaN.
 * Refused (-2) before anything is launched, writing nothing: a shape outside pmgt_dcn_train_grad's, n outside [1, PMGT_NCF_MAX_USERS],
 * n_items or rows < 1, row_stride < n_items, half not 0 or 1, a NULL or misaligned buffer (parameters, pu, pi, tables and row scalars: 16
 * bytes; users: 8; scores and consts: 4), a layer_norm_eps that is NaN, negative or infinite, more workgroups than a grid holds.
 * Added without a bump of pmgt_abi_version(): two entries, nothing existing moved. */
enum { PMGT_DCN_SCORE_ROW_STRIDE = 12 };             /* floats a row of pmgt_dcn_score_rows: a multiple of 4, at least PMGT_DCN_MAX_CROSS + 3 */
int pmgt_dcn_score_rows(const pmgt_dcn_head* head, const float* table, int64_t rows, int half, float* out, void* stream);
int pmgt_dcn_score(const pmgt_dcn_head* head, const float* pu, const float* pi, const float* user_rows, const float* item_rows,
                   const float* consts, const int64_t* users, int64_t n, int64_t n_items, float* scores, int64_t row_stride, void* stream);

/* Weight averaging ON THE DEVICE over the flat parameter buffer: the StochasticWeightAveraging callback's running mean
 * (pmgt/callbacks.py:44-381 over swa_init / swa_step / swap_swa_params, pmgt/utils/train.py:39-85) and a per-step exponential average
 * that lives inside a captured step.  One update is, per element,
 *   avg[j] = avg[j] * w_old + params[j] * w_new
 * in fp32 with THREE roundings (two products, one sum; never a fused multiply-add), so a numpy fp32 restatement matches bit for bit.
 *   PMGT_AVG_SWA  the caller passes both weights by value (the reference: beta = 1.0 / models_num, w_old = 1 - beta, w_new = beta, formed
 *                 in doubles and rounded to fp32 once); decay, warmup, state and skip_flag are ignored.  One launch.
 *   PMGT_AVG_EMA  the weights are computed on the device from the count of applied updates n_upd kept in `state`:
 *                 d = decay, or with warmup != 0 d = min(decay, (1 + n_upd) / (10 + n_upd)), in fp64; w_old = (float)d,
 *                 w_new = (float)(1.0 - d); then n_upd += 1.  skip_flag (device fp32 scalar, or NULL = never skipped) is the optimizer's
 *                 scal [5] of pmgt_optimizer_step_guarded: when it is non-zero the update is SKIPPED -- the skip word is set, n_upd and
 *                 every byte of avg stay as they were.  w_old / w_new of the struct are ignored.  Two launches (one lane that prepares,
 *                 then the update, which reads only what the earlier launch wrote), no sync, no allocation: capturable.
 * THE DEVICE STATE, PMGT_AVG_STATE_BYTES of 8-byte aligned device memory owned by the caller, zero-filled before the first update:
 *   bytes [0, 8)    int64  n_upd: updates applied so far (a skipped one does not count)
 *   bytes [8, 12)   uint32 skip word: 1 when the last update was skipped, else 0
 *   bytes [12, 16)  fp32   w_old of the last applied update
 *   bytes [16, 20)  fp32   w_new of the last applied update
 *   bytes [20, 32)  reserved, never touched
 * avg and params are device fp32 [n]; 16-byte aligned bases (any torch allocation) take 16-byte accesses, others a scalar form of the
 * same arithmetic.  Refused (-2): a NULL buffer or cfg, n < 0, an unknown mode, and in PMGT_AVG_EMA a decay outside [0, 1) or a NULL /
 * misaligned state.  n = 0 is valid (PMGT_AVG_EMA still counts the update).
 * Added without a bump of pmgt_abi_version(): the ABI grew by addition only (one struct, two entries), nothing existing moved. */
#define PMGT_AVG_SWA 0
#define PMGT_AVG_EMA 1
#define PMGT_AVG_STATE_BYTES 32
typedef struct pmgt_avg_step {
    int mode;                /* PMGT_AVG_* */
    int warmup;              /* PMGT_AVG_EMA: != 0 applies the warm-up of the decay */
    double decay;            /* PMGT_AVG_EMA: in [0, 1) */
    void* state;             /* PMGT_AVG_EMA: the device state above */
    const float* skip_flag;  /* PMGT_AVG_EMA: device fp32 scalar or NULL */
    float w_old, w_new;      /* PMGT_AVG_SWA: the two weights */
} pmgt_avg_step;
/* pmgt/utils/train.py:53-69 (swa_step) and the per-step form of the same update */
int pmgt_weight_average_update(float* avg, const float* params, int64_t n, const pmgt_avg_step* cfg, void* stream);
/* pmgt/utils/train.py:72-85 (swap_swa_params): exchanges the CONTENTS of a and b (device fp32 [n], not overlapping) as raw 32-bit words --
 * the engine, its captured steps and the nn.Parameter views address the parameter buffer by pointer, so the pointers cannot be exchanged
 * as the reference does.  Applying it twice restores both.  Refused (-2): a NULL buffer, n < 0, a == b. */
int pmgt_weight_swap(float* a, float* b, int64_t n, void* stream);

/* Gradient-ready notification for the data-parallel exchange (replaces DDP's autograd hooks + buckets,
 * pmgt/base_trainer.py:309-322 -> pl.Trainer(gpus=N)): during a backward pass the engine calls cb(user, offset, numel) on
 * the CALLING host thread right after it has enqueued the last launch that writes grads[offset, offset + numel) -- i.e.
 * work the callee enqueues on `stream` (an event record, an all-reduce that waits for that event) is ordered after those
 * writes and overlaps the rest of the backward pass.  Buckets arrive in backward order and tile the flat buffer exactly
 * once per backward call: NFR head (pmgt_pretrain_step only; pmgt_encode_backward produces no gradient for it and its
 * buckets tile the `bert.*` range), encoder layers L-1 .. 0, embeddings.  cb = NULL switches it off.  With the
 * options "side_stream_reduce" or "one_bucket" set, one bucket covering the whole buffer is reported at the end. */
typedef void (*pmgt_grad_ready_fn)(void* user, int64_t offset, int64_t numel);
void pmgt_engine_set_grad_ready_callback(pmgt_engine* e, pmgt_grad_ready_fn cb, void* user);

/* Per-phase timers (what the reference lacks entirely): between begin and end every group of
 * kernel launches is bracketed by HIP events on its stream; end() waits for them and writes one
 * "name count total_ms" line per phase into buf.  Off by default. */
int pmgt_profile_begin(pmgt_engine* e);
int pmgt_profile_end(pmgt_engine* e, char* buf, int cap);
/* the phases recorded so far, in launch order, one name per line (between begin and end; no wait) */
int pmgt_profile_sequence(pmgt_engine* e, char* buf, int cap);
/* the same records with their times, "name ms" per line in launch order (waits for the events; the records stay for pmgt_profile_end) */
int pmgt_profile_records(pmgt_engine* e, char* buf, int cap);

/* dtype plumbing */
int pmgt_cast_from_f32(int dtype, const float* src, void* dst, int64_t n, void* stream);
int pmgt_cast_to_f32(int dtype, const void* src, float* dst, int64_t n, void* stream);

/* fp8 mode plumbing: dst[i] = e4m3_rne(clamp(src[i] * inv_scale, +-448)) and back (n % 8 == 0).  The frozen tables are
 * quantised once by the caller with inv_scale = 448 / max|table|; table_scale = max|table| / 448. */
int pmgt_quantize_e4m3(const float* src, void* dst, int64_t n, float inv_scale, void* stream);
int pmgt_dequantize_e4m3(const void* src, float* dst, int64_t n, float scale, void* stream);

/* Path options: PER-ENGINE switches between the fused / streaming kernels of the product path and their plain
 * counterparts (parity A/B, bisecting).  key = one of the names listed in include/pmgt_ops.h ("store_ln_input",
 * "no_fused_attention_bwd", ...), value 0 = product path (default), 1 = alternative.  Returns 0, or -2 for an unknown key.
 * Options are state of THIS engine only: two engines in one process do not see each other's choices, and nothing in the
 * library reads the environment.  Set them before the first pmgt_workspace_bytes / step call of a shape (workspace
 * carving depends on some of them). */
int pmgt_engine_set_option(pmgt_engine* e, const char* key, int value);
/* current value (0 / 1), or -2 for an unknown key */
int pmgt_engine_get_option(const pmgt_engine* e, const char* key);

/* ---- host MCNSampling (libpmgt_sampler.so; pure host code, no HIP) --------------------------------
 * Replaces _sample_context_neigh / get_input_tensor / PMGTDataset.__getitem__ / pmgt_collate_fn
 * (pmgt/pmgt/datasets.py:14-208).  The graph is an ordered adjacency in CSR form: node ids 2..N+1
 * (0 = <pad>, 1 = <mask>), indptr has N+3 entries (rows 0 and 1 empty), neighbours in networkx
 * insertion order, float64 edge weights. */
typedef struct pmgt_sampler pmgt_sampler;
pmgt_sampler* pmgt_sampler_create(int64_t n_nodes, const int64_t* indptr, const int64_t* indices,
                                  const double* weights, const int* hop_sizes, int n_hops, int max_ctx_neigh,
                                  int max_total_samples, int min_neg_samples);
void pmgt_sampler_destroy(pmgt_sampler* s);
const char* pmgt_sampler_last_error(void);
/* np.random.seed(seed) of the reference's process-global legacy MT19937 stream (pmgt/utils/base.py:37). */
void pmgt_sampler_seed(pmgt_sampler* s, uint32_t seed);
/* One context: ids[S] (target first), mask[S]; returns num_ctx or <0 (datasets.py:64-79). */
int pmgt_sampler_context(pmgt_sampler* s, int64_t target, int64_t* ids, float* mask);
/* Collated batch in dataset order from ONE sequential stream (bit-exact with the reference run with
 * num_workers=0).  mode: 0 train, 1 eval, 2 inference.  pair buffers sized n*max_pairs(mode) rows.
 * Returns total pairs or <0. */
int pmgt_sampler_batch(pmgt_sampler* s, const int64_t* targets, int n, int mode, int64_t* tgt_ids, float* tgt_mask,
                       int64_t* pair_ids, float* pair_mask, int64_t* num_pairs, float* labels);
/* Same batch layout, sampled by n_threads host threads; target i gets its own stream seeded from
 * (base_seed, counter + counter_stride * i), so results do not depend on the thread count (statistical, not bit, parity
 * with the reference — the reference's own worker streams depend on the torch version).  counter_stride = 1
 * for consecutive items; a rank that evaluates items r, r + W, r + 2W, ... of a list passes counter = r (+ W * offset)
 * and counter_stride = W and so draws exactly what a single process draws for the same items. */
int pmgt_sampler_batch_mt(pmgt_sampler* s, const int64_t* targets, int n, int mode, uint64_t base_seed,
                          uint64_t counter, uint64_t counter_stride, int n_threads, int64_t* tgt_ids, float* tgt_mask, int64_t* pair_ids,
                          float* pair_mask, int64_t* num_pairs, float* labels);
int pmgt_sampler_max_pairs(const pmgt_sampler* s, int mode);
/* legacy-stream primitives exposed for tests */
double pmgt_sampler_random_sample(pmgt_sampler* s);
int64_t pmgt_sampler_randint(pmgt_sampler* s, int64_t n);
/* sklearn train_test_split(arange(2, N+2), test_size, random_state=seed) (pmgt/pmgt/trainer.py:45-52) */
int pmgt_train_valid_split(int64_t n_nodes, double valid_size, uint32_t seed, int64_t* train_out, int64_t* valid_out);

#ifdef __cplusplus
}
#endif
#endif /* PMGT_CAPI_H */
