// Training of the head of PMGT_NCF over an item table, FROZEN (pmgt_ncf_train_grad of include/pmgt_capi.h) or TRAINED WITH THE HEAD
// (pmgt_ncf_train_grad_table; the head: pmgt/pmgt_ncf/models.py:91-105, the step it serves: pmgt/ncf/trainer.py:183-200, the table's
// requires_grad_: pmgt/ncf/trainer.py:168-179): loss, logits and the gradient of the mean BCE-with-logits loss with respect to every
// parameter of the head -- and, for the second entry, to the table --, for n (user, item, label) pairs, in TWO launches.  Kept out of csrc/ for
// ncf_score.hip's reason: the measured step launches nothing of this.  The pair-major product forms, the roles rank / zero / weight / rows
// and the chain policies are stated in pair_train_tile.h; this file's products are Chain::ONE with the ReLU in the epilogue, and its loss
// line is the FUSED form of pair_bce (the file is compiled with the compiler's default contraction).
//
// LAUNCH 1, ncf_train_pairs_kernel: the roles rank (by user id and, NeuMF-end, by item id) and zero (the embedding gradients and, as a
// second range, the table's gradient), and
//   tile   32 pairs a workgroup: gathers [U_mlp[u] ; table[i]] on the fly, runs the layers, the GMF product and the predict layer, the loss
//          and dlogit, then walks back: dz_l = (W_(l+1)^T dz_(l+1)) * (act_l > 0) down to the user half of layer 0's input (frozen table:
//          dx [n][d]) or to all of it (trained table: dx [n][2 d], the item half behind the user half; a column block is computed on its
//          own, so the user half has the same bits either way).  Between layers the rows go through the workspace; a workgroup reads only
//          what it wrote itself, behind a barrier.
// LAUNCH 2, ncf_train_grads_kernel: the roles weight and rows.  The user kind of rows sums dx's user half and the GMF user rows, the item
// kind the GMF item rows (NeuMF-end) and, for a trained table, the item half of dx.
//
// DROPOUT (pmgt_ncf_train_grad_dropout; the DROP instantiations, the others are the kernels as they were): PMGT_NCF.head in training mode,
// the masks m = 0 or 1 / (1 - p) drawn by the counter-based RNG of csrc/common.h from the caller's device {seed, step} pair, indexed by
// (pair, feature), one hash pair per 4 neighbouring features, nothing stored:
//   emb      x0 = m_e [U_mlp[u] ; table[i]]: applied to the 16-byte x loads of layer 0, drawn again by the weight task of layer 0 in launch 2
//            (its B operand is gathered from the tables) and by the last data gradient, which makes dx the gradient of the embedding ROWS
//   layer l  act_l = m_l relu(W_l x + b_l) = relu(m_l (W_l x + b_l)): applied before the store.  The stored activation is > 0 exactly where
//            the element was kept and its pre-activation positive (the scale is >= 1), so the walk back keeps its act > 0 tests, multiplies
//            the passed gradient by 1 / (1 - p_l) and draws no layer mask again
//   gmf      gprod = m_g (gmf_u gmf_i), a mask of its own at emb_dropout's p: stored dropped, drawn again for the per-pair GMF gradients
// A site whose p is 0 draws nothing and multiplies by nothing.
//
// PER-PAIR ITEM ROWS (pmgt_ncf_train_grad_rows: the head on top of an encoder that is trained with it, every pair with a context and so an
// item embedding of its own), still TWO launches: the TABLE instantiations with two run-time differences.  Launch 1 reads the item half of
// layer 0's input from row `pair` of x_item [n][d] instead of table[items[pair]], and the weight task of layer 0 reads the same rows (PairSrc
// by the pair index).  Launch 2 sums no table rows; its extra role
//   item   copies the item half of dx [n][2 d] into the caller's d_item [n][d], 16 bytes a thread: one row per pair, nothing summed
// so two pairs on one item keep their own gradient rows.  The other entries launch no block of this role and keep their bits.
#include <climits>

#include "pair_train_tile.h"

namespace pmgt {

static constexpr int NT_MAX_LAYERS = PMGT_NCF_MAX_LAYERS, NT_MAX_TASKS = NT_MAX_LAYERS + 1;

struct NtLayer {
    const float* w;      // [out][2 out]
    const float* b;      // [out]
    float* act;          // workspace [n][out]: relu(W x + b)
    float* dz;           // workspace [n][out]: d loss / d (W x + b)
    int out;
};

struct NtPairsArgs {
    NtLayer layer[NT_MAX_LAYERS];
    const float *u_mlp, *table, *gu, *gi, *wp, *bp;
    const float* x_item;                     // rows entry: layer 0's item half of pair p is row p of this [n][d]; else NULL (table[items[p]])
    const int64_t *users, *items;
    const float* labels;
    float *dx, *gprod, *ggu, *ggi, *pz;      // workspace: [n][d] (trained table: [n][2 d]), [n][F] x 3, [n][2] = (dlogit, loss of the pair)
    int *order_u, *order_i;                  // workspace: the pairs in stable order by user / item id
    float* logits;                           // [n] or NULL
    float* zero_base;                        // the embedding gradients
    int64_t zero_vec4;                       // ... in 16-byte pieces
    float* zero2_base;                       // the table's gradient (trained table), a second range
    int64_t zero2_vec4;                      // ... in 16-byte pieces; 0: no second range
    int n, d, factor, num_layers, neumf, tiles, rank_blocks, zero_blocks;
};

typedef pmgt_ncf_dropout NtDrop;      // the second kernel argument; only the DROP instantiations read it

struct NtGradsArgs {
    PairTask task[NT_MAX_TASKS];
    const int64_t *users, *items;
    const int *order_u, *order_i;
    const float *dx, *ggu, *ggi;
    float *g_u_mlp, *g_gu, *g_gi, *g_table, *loss;                   // g_table: the trained table's gradient, else NULL
    float* d_item;                                                   // rows entry: [n][d], the item half of dx per pair; else NULL
    int n, d, factor, neumf, ntasks, weight_blocks, row_blocks;      // row_blocks per kind (user, item)
    int item_first, item_blocks;                                     // rows entry: the first block and the count of the `item` role; else (INT_MAX, 0)
};

// TABLE: the item table is trained (the frozen instantiation is the kernel as it was: the widths below fold to d)
// DROP: dropout is on at one site or more (without it the kernel's instructions are those it had: `dr` is not read)
template <bool TABLE, bool DROP>
__global__ __launch_bounds__(PAIR_THREADS) void ncf_train_pairs_kernel(NtPairsArgs a, NtDrop dr) {
    __shared__ float s_dl[PAIR_TILE];
    __shared__ int64_t s_ids[PAIR_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = pair_wave_index(), n = a.n;
    int bid = blockIdx.x;
    if (bid >= a.tiles + 2 * a.rank_blocks) {                // ---- zero: the embedding gradients, whole, and the table's
        pair_zero<TABLE>(bid - a.tiles - 2 * a.rank_blocks, a.zero_blocks, a.zero_base, a.zero_vec4, a.zero2_base, a.zero2_vec4, tid);
        return;
    }
    if (bid >= a.tiles) {                                    // ---- rank: the stable order by id, counted
        pair_rank(bid - a.tiles, a.rank_blocks, n, a.users, a.items, a.order_u, a.order_i, s_ids, tid);
        return;
    }
    // ---- tile: forward and data gradient of 32 pairs
    const int d = a.d, F = a.factor, L = a.num_layers;
    const int pl = lane & 31, h = lane >> 5;
    const int pair = bid * PAIR_TILE + pl;
    const bool valid = pair < n;
    const int64_t uid = valid ? a.users[pair] : 0, iid = valid ? a.items[pair] : 0;
    const float* urow = a.u_mlp + uid * d;
    const float* irow = a.x_item ? a.x_item + (int64_t)pair * d : a.table + iid * d;
    DropKey kemb = pair_drop_off(), kgmf = pair_drop_off(), klay = pair_drop_off();
    if constexpr (DROP) {
        kemb = make_drop_key(DropCfg{dr.rng, dr.p_emb, NCF_SITE_EMB});
        if (a.neumf) kgmf = make_drop_key(DropCfg{dr.rng, dr.p_emb, NCF_SITE_GMF});
        klay = make_drop_key(DropCfg{dr.rng, dr.p_layer[0], NCF_SITE_LAYER});
    }
    pair_linear<Chain::ONE, true, DROP>(a.layer[0].w, a.layer[0].b, d, 2 * d, urow, d, irow, valid, a.layer[0].act + (int64_t)pair * d, wave, lane,
                                        kemb, klay, pair);
    __syncthreads();
    for (int l = 1; l < L; ++l) {
        const int M = a.layer[l].out;
        if constexpr (DROP) klay = make_drop_key(DropCfg{dr.rng, dr.p_layer[l], NCF_SITE_LAYER + (uint32_t)l});
        pair_linear<Chain::ONE, true, DROP>(a.layer[l].w, a.layer[l].b, M, 2 * M, a.layer[l - 1].act + (int64_t)pair * 2 * M, 2 * M, nullptr, valid,
                                            a.layer[l].act + (int64_t)pair * M, wave, lane, pair_drop_off(), klay, pair);
        __syncthreads();
    }
    const float* feat = a.layer[L - 1].act;                  // [n][F]
    const float* wp_mlp = a.wp + (a.neumf ? F : 0);
    if (wave == 0) {                                         // predict layer, loss, dlogit: a pair on lanes p and p + 32, half the factors each
        float s = 0.f;
        if (valid) {
            const int half = F >> 1;
            if (a.neumf) {
                const float* gu = a.gu + uid * F;
                const float* gi = a.gi + iid * F;
                if constexpr (DROP) {                        // (half is a multiple of 4: one draw per 4 factors)
                    for (int f = h * half; f < (h + 1) * half; f += 4) {
                        float mk[4] = {1.f, 1.f, 1.f, 1.f};
                        if (kgmf.on) drop_mul4(kgmf, (uint32_t)pair, (uint32_t)(f >> 2), mk);
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            const float g = gu[f + e] * gi[f + e] * mk[e];
                            a.gprod[(int64_t)pair * F + f + e] = g;
                            s = fmaf(a.wp[f + e], g, s);
                        }
                    }
                } else {
                    for (int f = h * half; f < (h + 1) * half; ++f) {
                        const float g = gu[f] * gi[f];
                        a.gprod[(int64_t)pair * F + f] = g;
                        s = fmaf(a.wp[f], g, s);
                    }
                }
            }
            const float* hl = feat + (int64_t)pair * F;
            for (int f = h * half; f < (h + 1) * half; ++f) s = fmaf(wp_mlp[f], hl[f], s);
        }
        s += __shfl_xor(s, 32, 64);
        if (h == 0) {
            float dl = 0.f;
            if (valid) {
                const float z = s + a.bp[0];
                float loss;
                pair_bce<true>(z, a.labels[pair], n, dl, loss);
                if (a.logits) a.logits[pair] = z;
                a.pz[(int64_t)pair * 2] = dl;
                a.pz[(int64_t)pair * 2 + 1] = loss;
            }
            s_dl[pl] = dl;
        }
    }
    __syncthreads();
    float gscale = 1.f;                                      // DROP: 1 / (1 - p) of the layer whose activation masks the gradient
    if constexpr (DROP) gscale = klay.scale;                 // (klay is the last layer's key)
    for (int e = tid; e < PAIR_TILE * F; e += PAIR_THREADS) {    // dz of the last layer and the per-pair GMF gradients
        const int pp = e / F, f = e - pp * F, pr = bid * PAIR_TILE + pp;
        if (pr >= n) continue;
        const float dl = s_dl[pp];
        const int64_t at = (int64_t)pr * F + f;
        if constexpr (DROP) a.layer[L - 1].dz[at] = feat[at] > 0.f ? dl * wp_mlp[f] * gscale : 0.f;
        else a.layer[L - 1].dz[at] = feat[at] > 0.f ? dl * wp_mlp[f] : 0.f;
        if (a.neumf) {
            float dg = dl * a.wp[f];
            if constexpr (DROP) {
                if (kgmf.on) dg *= drop_mul1(kgmf, (uint32_t)pr, (uint32_t)f);
            }
            a.ggu[at] = dg * a.gi[a.items[pr] * F + f];
            a.ggi[at] = dg * a.gu[a.users[pr] * F + f];
        }
    }
    __syncthreads();
    for (int l = L - 1; l >= 1; --l) {
        const int M = a.layer[l].out;
        if constexpr (DROP) gscale = make_drop_key(DropCfg{dr.rng, dr.p_layer[l - 1], NCF_SITE_LAYER + (uint32_t)(l - 1)}).scale;
        pair_linear_bwd<Chain::ONE, DROP>(a.layer[l].w, M, 2 * M, 2 * M, a.layer[l].dz + (int64_t)pair * M,
                                          a.layer[l - 1].act + (int64_t)pair * 2 * M, valid, a.layer[l - 1].dz + (int64_t)pair * 2 * M, wave, lane,
                                          gscale, pair_drop_off(), pair);
        __syncthreads();
    }
    const int dxw = TABLE ? 2 * d : d;                       // the columns of layer 0's input that dx covers
    pair_linear_bwd<Chain::ONE, DROP>(a.layer[0].w, d, 2 * d, dxw, a.layer[0].dz + (int64_t)pair * d, nullptr, valid, a.dx + (int64_t)pair * dxw,
                                      wave, lane, 1.f, kemb, pair);
}

// DROP: the weight task of layer 0 gathers its B operand from the tables and applies the emb mask to it, drawn again per element
template <bool TABLE, bool DROP>
// 7 waves a SIMD (72 VGPRs), the occupancy of the DROP instantiations before the weight role was shared (68 VGPRs; the plain ones had 80 and 6
// waves): unbounded, the DROP instantiations take 73, one over; the plain ones need 67 either way
__global__ __launch_bounds__(PAIR_THREADS, 7) void ncf_train_grads_kernel(NtGradsArgs a, NtDrop dr) {
    __shared__ float s_acc[PAIR_WAVES][16][64];
    const int tid = threadIdx.x, lane = tid & 63, wave = pair_wave_index(), n = a.n;
    int bid = blockIdx.x;
    if (bid >= a.item_first) {                               // ---- item (rows entry): d_item [n][d] = the item half of dx [n][2 d], 16 bytes a thread
        const int q = a.d >> 2;                              // (d is a multiple of 8)
        const float4* src = reinterpret_cast<const float4*>(a.dx);
        float4* dst = reinterpret_cast<float4*>(a.d_item);
        for (int64_t i = (int64_t)(bid - a.item_first) * PAIR_THREADS + tid; i < (int64_t)n * q; i += (int64_t)a.item_blocks * PAIR_THREADS) {
            const int64_t pr = i / q;
            dst[i] = src[pr * 2 * q + q + (i - pr * q)];
        }
        return;
    }
    if (bid >= a.weight_blocks) {                            // ---- rows: segment sums of the per-pair embedding gradients in pair order
        const PairRun r = pair_run(bid - a.weight_blocks, a.row_blocks, wave, n, a.users, a.items, a.order_u, a.order_i);
        if (!r.start) return;
        const int kind = r.kind;
        const int d = a.d, F = a.factor;
        const int Fg = a.neumf ? F : 0;                      // the GMF rows of this kind
        const int dxw = TABLE ? 2 * d : d;
        const int width = kind ? Fg + (TABLE && a.g_table ? d : 0) : d + Fg;      // (the rows entry has dx [n][2 d] and no table to sum into)
        for (int c = lane; c < width; c += 64) {
            const float* src;                                // the per-pair rows, `sw` floats apart
            float* dst;                                      // the table's rows, `w` floats wide
            int sw, w, cc;
            if (kind) {
                if (c < Fg) { src = a.ggi; dst = a.g_gi; sw = w = F; cc = c; }
                else { src = a.dx + d; dst = a.g_table; sw = dxw; w = d; cc = c - Fg; }
            }
            else if (c < d) { src = a.dx; dst = a.g_u_mlp; sw = dxw; w = d; cc = c; }
            else { src = a.ggu; dst = a.g_gu; sw = w = F; cc = c - d; }
            dst[r.id * w + cc] = pair_run_sum(r, n, src, sw, cc);
        }
        return;
    }
    // ---- weight: one 32 x 32 block of dW = dz^T x, the pairs in order
    pair_weight_block<DROP, true>(a.task, a.ntasks, bid, n, a.loss, DropCfg{dr.rng, dr.p_emb, NCF_SITE_EMB}, s_acc, tid, lane, wave);
}

struct NtShape {
    int F, L, d, neumf;
    int64_t user_num, item_num;
};

static int nt_shape(int factor_num, int num_layers, int kind, int64_t user_num, int64_t item_num, const char* who, NtShape* s) {
    int d;
    if (int rc = ncf_head_check(factor_num, num_layers, kind, who, &d)) return rc;
    if (int rc = pair_check_rows(who, user_num, item_num)) return rc;
    *s = NtShape{factor_num, num_layers, d, kind == PMGT_NCF_NEUMF_END, user_num, item_num};
    return 0;
}

// the flat parameter layout: off[PMGT_NCF_TRAIN_TENSORS] in floats (-1 = the head has no such tensor) -> the parameter count
static int64_t nt_layout(const NtShape& s, int64_t* off) {
    int64_t at = 0;
    for (int i = 0; i < PMGT_NCF_TRAIN_TENSORS; ++i) off[i] = -1;
    off[0] = at, at += s.user_num * s.d;
    if (s.neumf) {
        off[1] = at, at += s.user_num * s.F;
        off[2] = at, at += s.item_num * s.F;
    }
    for (int l = 0; l < s.L; ++l) {
        const int64_t out = s.d >> l;
        off[3 + 2 * l] = at, at += out * 2 * out;
        off[4 + 2 * l] = at, at += out;
    }
    off[3 + 2 * NT_MAX_LAYERS] = at, at += s.neumf ? 2 * s.F : s.F;
    off[4 + 2 * NT_MAX_LAYERS] = at, at += 1;
    return at;
}

// the workspace in floats: act_l and dz_l [n][d >> l], dx [n][d] (trained table: [n][2 d]), gprod / ggu / ggi [n][F], pz [n][2], then the
// two orders (int [n] each)
static int64_t nt_workspace_floats(const NtShape& s, int64_t n, bool table) {
    int64_t w = 0;
    for (int l = 0; l < s.L; ++l) w += 2 * n * (s.d >> l);
    w += n * s.d * (table ? 2 : 1) + 3 * n * s.F;
    w += (2 * n + 3) / 4 * 4;
    w += 2 * ((n + 3) / 4 * 4);
    return w;
}

}  // namespace pmgt

using namespace pmgt;

extern "C" {

int64_t pmgt_ncf_train_layout(int factor_num, int num_layers, int kind, int64_t user_num, int64_t item_num, int64_t* offsets) {
    NtShape s;
    if (int rc = nt_shape(factor_num, num_layers, kind, user_num, item_num, "pmgt_ncf_train_layout", &s)) return rc;
    int64_t off[PMGT_NCF_TRAIN_TENSORS];
    const int64_t count = nt_layout(s, off);
    if (offsets)
        for (int i = 0; i < PMGT_NCF_TRAIN_TENSORS; ++i) offsets[i] = off[i];
    return count;
}

}  // extern "C"

namespace pmgt {

static int64_t nt_workspace_bytes(int factor_num, int num_layers, int kind, int64_t n, bool table, const char* who) {
    NtShape s;
    if (int rc = nt_shape(factor_num, num_layers, kind, 1, 1, who, &s)) return rc;
    if (int rc = pair_check_n(who, n, PMGT_NCF_TRAIN_MAX_PAIRS)) return rc;
    return nt_workspace_floats(s, n, table) * (int64_t)sizeof(float);
}

// every gradient entry; want_table: the table is trained and table_grad [item_num][d] is written whole; drop: NULL or the dropout of the call;
// rows: the rows entry -- layer 0's item half is x_item [n][d] by the pair index, head->table is not read, d_item [n][d] is written whole
static int nt_grad(const char* who, const pmgt_ncf_train* head, const int64_t* users, const int64_t* items, const float* labels, int64_t n,
                   float* loss, float* logits, bool want_table, float* table_grad, const pmgt_ncf_dropout* drop, void* workspace,
                   int64_t workspace_bytes, void* stream, bool rows = false, const float* x_item = nullptr, float* d_item = nullptr) {
    PMGT_CHECK(head != nullptr, -2, "%s: NULL head", who);
    NtShape s;
    if (int rc = nt_shape(head->factor_num, head->num_layers, head->kind, head->user_num, head->item_num, who, &s)) return rc;
    if (int rc = pair_check_n(who, n, PMGT_NCF_TRAIN_MAX_PAIRS)) return rc;
    PMGT_CHECK((rows || head->table) && head->params && head->grads && users && items && labels && loss && workspace, -2, "%s: NULL buffer", who);
    PMGT_CHECK(!want_table || table_grad, -2, "%s: NULL table_grad", who);
    PMGT_CHECK(!rows || (x_item && d_item), -2, "%s: NULL x_item or d_item", who);
    const uintptr_t table_bits = rows ? ((uintptr_t)x_item | (uintptr_t)d_item) : (uintptr_t)head->table;
    PMGT_CHECK(((table_bits | (uintptr_t)head->params | (uintptr_t)head->grads | (uintptr_t)workspace | (uintptr_t)table_grad) & 15) == 0, -2,
               "%s: the table (the rows entry: x_item and d_item), the parameters, the gradients (the table's included) and the workspace must be "
               "16-byte aligned", who);
    if (int rc = pair_check_small(who, users, items, labels, loss, logits)) return rc;
    const bool wide = want_table || rows;                    // dx covers all 2 d columns of layer 0's input
    const int64_t need = nt_workspace_floats(s, n, wide) * (int64_t)sizeof(float);
    PMGT_CHECK(workspace_bytes >= need, -2, "%s: workspace of %lld bytes below the %lld needed", who, (long long)workspace_bytes, (long long)need);
    NtDrop dr;
    bool drop_on;                                            // every p 0: the instantiations without dropout
    if (int rc = pair_check_ncf_dropout(who, drop, s.L, &dr, &drop_on)) return rc;
    int64_t off[PMGT_NCF_TRAIN_TENSORS];
    nt_layout(s, off);
    const float* P = head->params;
    float* G = head->grads;
    float* ws = (float*)workspace;
    const int F = s.F, L = s.L, d = s.d;
    const int OFF_WP = 3 + 2 * NT_MAX_LAYERS, OFF_BP = 4 + 2 * NT_MAX_LAYERS;

    NtPairsArgs pa = {};
    NtGradsArgs ga = {};
    for (int l = 0; l < L; ++l) {
        const int out = d >> l;
        pa.layer[l].w = P + off[3 + 2 * l];
        pa.layer[l].b = P + off[4 + 2 * l];
        pa.layer[l].out = out;
        pa.layer[l].act = ws, ws += n * out;
        pa.layer[l].dz = ws, ws += n * out;
    }
    const int dxw = wide ? 2 * d : d;
    pa.dx = ws, ws += n * dxw;
    pa.gprod = ws, ws += n * F;
    pa.ggu = ws, ws += n * F;
    pa.ggi = ws, ws += n * F;
    pa.pz = ws, ws += (2 * n + 3) / 4 * 4;
    pa.order_u = (int*)ws, ws += (n + 3) / 4 * 4;
    pa.order_i = (int*)ws;
    pa.u_mlp = P + off[0];
    pa.table = rows ? nullptr : head->table;
    pa.x_item = x_item;
    pa.gu = s.neumf ? P + off[1] : nullptr;
    pa.gi = s.neumf ? P + off[2] : nullptr;
    pa.wp = P + off[OFF_WP];
    pa.bp = P + off[OFF_BP];
    pa.users = users;
    pa.items = items;
    pa.labels = labels;
    pa.logits = logits;
    pa.zero_base = G;
    pa.zero_vec4 = off[3] / 4;                               // the embedding tables come first; every size is a multiple of 8 floats
    pa.zero2_base = table_grad;
    pa.zero2_vec4 = want_table ? s.item_num * d / 4 : 0;     // (d is a multiple of 8)
    pa.n = (int)n, pa.d = d, pa.factor = F, pa.num_layers = L, pa.neumf = s.neumf;
    pa.tiles = (int)cdiv64(n, PAIR_TILE);
    pa.rank_blocks = (int)cdiv64(n, PAIR_THREADS);
    pa.zero_blocks = (int)std::min<int64_t>(PAIR_ZERO_BLOCKS, cdiv64(pa.zero_vec4 + pa.zero2_vec4, PAIR_THREADS));

    int first = 0;
    for (int l = 0; l < L; ++l) {
        const int out = d >> l;
        const PairSrc x0 = rows ? PairSrc{pa.u_mlp, users, d, x_item, nullptr, d} : PairSrc{pa.u_mlp, users, d, pa.table, items, d};
        pair_add_task(ga.task, &ga.ntasks, &first, pa.layer[l].dz, out, l == 0 ? x0 : PairSrc{pa.layer[l - 1].act, nullptr, 2 * out, nullptr, nullptr, 0},
                      G + off[3 + 2 * l], G + off[4 + 2 * l], false);
    }
    pair_add_task(ga.task, &ga.ntasks, &first, pa.pz, 2,
                  s.neumf ? PairSrc{pa.gprod, nullptr, F, pa.layer[L - 1].act, nullptr, F} : PairSrc{pa.layer[L - 1].act, nullptr, F, nullptr, nullptr, 0},
                  G + off[OFF_WP], G + off[OFF_BP], true);
    ga.weight_blocks = first;
    ga.row_blocks = (int)cdiv64(n, PAIR_WAVES);
    ga.users = users, ga.items = items;
    ga.order_u = pa.order_u, ga.order_i = pa.order_i;
    ga.dx = pa.dx, ga.ggu = pa.ggu, ga.ggi = pa.ggi;
    ga.g_u_mlp = G + off[0];
    ga.g_gu = s.neumf ? G + off[1] : nullptr;
    ga.g_gi = s.neumf ? G + off[2] : nullptr;
    ga.g_table = want_table ? table_grad : nullptr;
    ga.loss = loss;
    ga.n = (int)n, ga.d = d, ga.factor = F, ga.neumf = s.neumf;

    hipStream_t st = (hipStream_t)stream;
    const int kinds = (s.neumf || want_table) ? 2 : 1;       // MLP over a frozen table has no rows indexed by item: its item order is not read
    ga.d_item = d_item;
    ga.item_first = rows ? ga.weight_blocks + kinds * ga.row_blocks : INT_MAX;
    ga.item_blocks = rows ? (int)std::min<int64_t>(PAIR_ZERO_BLOCKS, cdiv64(n * (d / 4), PAIR_THREADS)) : 0;
    const unsigned grid1 = (unsigned)(pa.tiles + 2 * pa.rank_blocks + pa.zero_blocks);
    if (drop_on) {
        if (wide) hipLaunchKernelGGL((ncf_train_pairs_kernel<true, true>), dim3(grid1), dim3(PAIR_THREADS), 0, st, pa, dr);
        else hipLaunchKernelGGL((ncf_train_pairs_kernel<false, true>), dim3(grid1), dim3(PAIR_THREADS), 0, st, pa, dr);
    }
    else if (wide) hipLaunchKernelGGL((ncf_train_pairs_kernel<true, false>), dim3(grid1), dim3(PAIR_THREADS), 0, st, pa, dr);
    else hipLaunchKernelGGL((ncf_train_pairs_kernel<false, false>), dim3(grid1), dim3(PAIR_THREADS), 0, st, pa, dr);
    PMGT_LAUNCH_OK();
    const unsigned grid2 = (unsigned)(ga.weight_blocks + kinds * ga.row_blocks + ga.item_blocks);
    if (drop_on && dr.p_emb > 0.f) {                         // (launch 2 draws the emb mask only)
        if (wide) hipLaunchKernelGGL((ncf_train_grads_kernel<true, true>), dim3(grid2), dim3(PAIR_THREADS), 0, st, ga, dr);
        else hipLaunchKernelGGL((ncf_train_grads_kernel<false, true>), dim3(grid2), dim3(PAIR_THREADS), 0, st, ga, dr);
    }
    else if (wide) hipLaunchKernelGGL((ncf_train_grads_kernel<true, false>), dim3(grid2), dim3(PAIR_THREADS), 0, st, ga, dr);
    else hipLaunchKernelGGL((ncf_train_grads_kernel<false, false>), dim3(grid2), dim3(PAIR_THREADS), 0, st, ga, dr);
    PMGT_LAUNCH_OK();
    return 0;
}

}  // namespace pmgt

extern "C" {

int64_t pmgt_ncf_train_workspace_bytes(int factor_num, int num_layers, int kind, int64_t n) {
    return nt_workspace_bytes(factor_num, num_layers, kind, n, false, "pmgt_ncf_train_workspace_bytes");
}

int64_t pmgt_ncf_train_table_workspace_bytes(int factor_num, int num_layers, int kind, int64_t n) {
    return nt_workspace_bytes(factor_num, num_layers, kind, n, true, "pmgt_ncf_train_table_workspace_bytes");
}

int pmgt_ncf_train_grad(const pmgt_ncf_train* head, const int64_t* users, const int64_t* items, const float* labels, int64_t n, float* loss,
                        float* logits, void* workspace, int64_t workspace_bytes, void* stream) {
    return nt_grad("pmgt_ncf_train_grad", head, users, items, labels, n, loss, logits, false, nullptr, nullptr, workspace, workspace_bytes, stream);
}

int pmgt_ncf_train_grad_table(const pmgt_ncf_train* head, const int64_t* users, const int64_t* items, const float* labels, int64_t n, float* loss,
                              float* logits, float* table_grad, void* workspace, int64_t workspace_bytes, void* stream) {
    return nt_grad("pmgt_ncf_train_grad_table", head, users, items, labels, n, loss, logits, true, table_grad, nullptr, workspace, workspace_bytes,
                   stream);
}

int pmgt_ncf_train_grad_dropout(const pmgt_ncf_train* head, const int64_t* users, const int64_t* items, const float* labels, int64_t n,
                                float* loss, float* logits, float* table_grad, const pmgt_ncf_dropout* drop, void* workspace,
                                int64_t workspace_bytes, void* stream) {
    const char* who = "pmgt_ncf_train_grad_dropout";
    PMGT_CHECK(drop != nullptr, -2, "%s: NULL drop", who);
    return nt_grad(who, head, users, items, labels, n, loss, logits, table_grad != nullptr, table_grad, drop, workspace, workspace_bytes, stream);
}

int64_t pmgt_ncf_train_rows_workspace_bytes(int factor_num, int num_layers, int kind, int64_t n) {
    return nt_workspace_bytes(factor_num, num_layers, kind, n, true, "pmgt_ncf_train_rows_workspace_bytes");
}

int pmgt_ncf_train_grad_rows(const pmgt_ncf_train* head, const int64_t* users, const int64_t* items, const float* labels, int64_t n, float* loss,
                             float* logits, const float* x_item, float* d_item, const pmgt_ncf_dropout* drop, void* workspace,
                             int64_t workspace_bytes, void* stream) {
    return nt_grad("pmgt_ncf_train_grad_rows", head, users, items, labels, n, loss, logits, false, nullptr, drop, workspace, workspace_bytes,
                   stream, true, x_item, d_item);
}

}  // extern "C"
