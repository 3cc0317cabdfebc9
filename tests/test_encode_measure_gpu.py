"""The inference entry of the engine (Engine.encode, the C ABI's pmgt_encode_ids / pmgt_encode_feats) held to measured noise and to its
invariants -- what export_embeddings, encode_catalogue, the catalogue scorers, similar_items, recommend_from_history and every
evaluate_* path read.

THE MEASURE is tests/encode_measure_util.py's `forward_ratios`: last_hidden_state, every hidden_states[i] and the attention probabilities
(where a case requests them) in max-abs and L2, the CLS rows last[:, 0] per sequence, against the oracle in fp64 (o64) with the yardstick
e16 (the oracle under the bf16 storage hook) for the bf16 engine and r32 (the oracle in float32 on the CPU) for the fp32 engine, each
error at most C_BOUND = 4 yardsticks floored at 2^-22 max|o64|; a key with mask 0 has probability == 0.0.  The engine reports the
probabilities from its fp32 registers BEFORE it packs them to bf16 for P V (see the util's header), so the hook hands back the value
from before its rounding.  tests/test_encode_measure_cpu.py settles the yardstick on the CPU with a second bf16 realisation.

CASES (encode_measure_util.CASES), each the smallest batch that selects its kernels; the bf16 run asserts the families in its launch
trace.  Every case: ragged masks with position 0 valid (one sequence keeps position 0 alone), dropout 0.1 in the config (inference must
ignore it), po.synth_params / po.synth_tables, every LayerNorm's gamma and beta randomised.
  headline    d = I = 256, H 8, L 2, S 32, beta 0.5; table mode (14 / 2 000 nodes) and token mode (5 000 nodes), Tseq
              1 (no fused kernel, tile GEMMs), 2 and 3 (fused; an odd count gives a half-empty last step), 255 (8 160 tokens, gemm_ws),
              256 (8 192, gemm_wsr), 257 and 258 (ragged last row tile)
  variants    beta = 1 at 256 (qkvc_attn_fwd_vc); attention_mask=None at 3 and 256; the feats= entry at 3 and 256;
              output_attentions at 3 (unfused path, probabilities measured); d 128 / H 2 / L 1 / S 65 with probabilities
  d = 512     H 8, S 64, L 2, Tseq 64 and 65: gemm_rowln, attn_tiles_fwd
  I = 4 d     d 256 / I 1 024, Tseq 761 (96 tiles of 256 rows): nt_lnf.  Its fp64 reference pair takes 3.5 s on 8 cores against the
              7.8 s of the step measure's I = 4 d case: not `slow`
  drivers     export_embeddings and encode_catalogue on 257 items at batch 128 (a last batch of ONE sequence): the same bits, the bits
              of encode's CLS rows batch by batch, and inside the row measure against the oracle on the same sampled contexts
  controls    the truth mis-stated at beta 0.53 (rejected on the probabilities; the hidden states move by less than bf16 noise, see
              the CPU file) and one sequence's rows overwritten with its neighbour's (rejected by the CLS-row kind -- and by the
              global max and L2 kinds alone, as the CPU file reports)

INVARIANTS, compared with == on bits at the headline shape, Tseq 3 and 257, table and token mode, bf16 and fp32: repeatable over a
workspace filled with 0xFF; encode draws nothing (rng_state, and a dropout-on pretrain_step after it has the bits of one on an engine
that never encoded); sequence order (a permuted batch, and one sequence inside two different batches); node ids at masked positions do
not reach a row at a valid position; hidden_states[L] is last_hidden_state and the plain call's.

Largest ratio per case measured on the MI355X (one run; bf16 against e16 / fp32 against r32):
  headline table mode   Tseq 1 1.00 / 3.58, 2 1.00 / 3.58, 3 1.00 / 3.43, 255 .. 258 1.12 / 2.84
  headline token mode   Tseq 1 1.00 / 2.70, 2 1.01 / 2.46, 3 1.01 / 3.59, 255 .. 258 1.09 / 2.52
  beta = 1 1.08 / 2.88; no mask 3: 1.75 / 3.65, 256: 1.16 / 3.03; feats 3: 1.01 / 3.59, 256: 1.09 / 2.52; probabilities at S 32 1.01 / 2.28,
  at d 128 / S 65 1.06 / 3.18; d = 512 1.05 / 1.97 at both counts; I = 4 d 1.17 / 3.71; drivers 1.11 / 2.16.
The bf16 engine rounds where the hook rounds, so its error IS e16's (ratios of 1.00; the largest a CLS row or a max-abs); the fp32
figures are max-abs errors of hidden_states.0 / .1 or the CLS rows against a single run of the oracle in float32 (L2 ratios stay below 1).
The second realisation on the CPU: at most 1.51 (tests/test_encode_measure_cpu.py).  Negative controls on the engine's output: beta 0.53
12.1 / 9.5 on probs.0 max / L2 (7.1 / 7.4 on probs.1); a mis-paired sequence 165 on its CLS row, and 89 / 12 on the global max / L2 of
the CLS table at 257 sequences.  The whole file: 93 tests in 12 s, the I = 4 d bf16 case 3.8 s of it, every other case below 0.7 s."""
import gc
import types

import numpy as np
import pytest
import torch

from oracle import pmgt_oracle as po
from tests import encode_measure_util as em
from tests.test_bf16_step_measure_gpu import dev_batch, launch_counts

pytestmark = pytest.mark.gpu

DTYPES = ("bf16", "fp32")
FAMILIES = ("qkvc_attn_fwd", "qkvc_attn_fwd_vc", "gemm_ws", "gemm_wsr", "nt_tile", "embed_tok8", "gemm_rowln", "attn_tiles_fwd", "nt_lnf")


def new_engine(cfg, params, tables, dtype):
    from pmgt_amd.configuration_pmgt import PMGTConfig
    from pmgt_amd.engine import Engine
    eng = Engine(PMGTConfig(**cfg), dtype=dtype, seed=0)
    eng.load_params(params)
    eng.set_tables(*[t.numpy() for t in tables])
    return eng


def engine(world_name, dtype):
    """a fresh engine on a world; no engine outlives its test (each owns a stream of its own and device buffers)"""
    w = em.world(world_name)
    return new_engine(w["cfg"], w["params"], w["tables"], dtype)


@pytest.fixture(scope="module", autouse=True)
def release_the_references_with_the_module():
    """the worlds and their references are shared by the tests of this file and dropped with it: nothing of it stays in the process"""
    yield
    for cached in (em.reference, em.world, em.misstated_truth):
        cached.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


def encode(eng, w, n_seq, entry="ids", hidden=True, probs=None, ids=None, mask="own"):
    """Engine.encode on the first n_seq sequences of the world (or on ids / mask given) -> (last, hs, pr), the launch trace reset before"""
    from pmgt_amd import _lib
    ids = w["ids"][:n_seq] if ids is None else ids
    mask = (None if w["mask"] is None else w["mask"][:n_seq]) if isinstance(mask, str) else mask
    m = None if mask is None else mask.cuda()
    probs = w["probs"] if probs is None else probs
    _lib.hip().pmgt_launch_trace_reset()
    if entry == "feats":
        feats = [f.cuda() for f in po.gather_feats(ids, w["tables"])]
        out = eng.encode(feats=feats, attention_mask=m, output_hidden_states=hidden, output_attentions=probs)
    else:
        out = eng.encode(ids=ids.cuda(), attention_mask=m, output_hidden_states=hidden, output_attentions=probs)
    torch.cuda.synchronize()
    return out


def engine_quantities(last, hs, pr):
    return em.quantities(last, list(hs), None if pr is None else list(pr))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ---- 1. the measure -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("label", list(em.CASES))
def test_encode_within_the_forward_measure(label, dtype):
    c = em.CASES[label]
    w, n_seq, o64, y, mask = em.case_truth(label, dtype)
    got = engine_quantities(*encode(engine(c["world"], dtype), w, n_seq, c.get("entry", "ids")))
    ran = launch_counts(FAMILIES)
    if dtype == "bf16":
        assert all(ran[k] >= 1 for k in c["expect"]) and all(ran[k] == 0 for k in c["absent"]), (label, ran)
    else:
        assert ran["qkvc_attn_fwd"] == 0 and ran["gemm_wsr"] == 0, ran
    rt = em.forward_ratios(got, o64, y, mask)
    print(f"encode measure {label} {dtype}: {n_seq * w['S']} tokens, {len(rt)} ratios, worst {em.worst(rt)}")
    assert not em.failing(rt), (label, dtype, em.failing(rt))


# ---- drivers --------------------------------------------------------------------------------------------------------------------------------
N_ITEMS, BATCH = 257, 128


def catalogue_graph():
    """257 nodes in rings with chords of 100, 100, 19, 19 and 19 nodes: sparse enough that the sampler's hops never collect 31 distinct
    neighbours, so every context is right-padded and masked (more than half of each batch) -- the single sequence of the last batch included"""
    from pmgt_amd.graph import CSRGraph
    edges, lo = [], 0
    for m in (100, 100, 19, 19, 19):
        edges += [np.stack([np.arange(m), (np.arange(m) + 1) % m], 1) + lo, np.stack([np.arange(0, m - 5, 3), np.arange(0, m - 5, 3) + 5], 1) + lo]
        lo += m
    assert lo == N_ITEMS
    e = np.concatenate(edges).astype(np.int64)
    return CSRGraph.from_edge_list(N_ITEMS, e + 2, 0.2 + np.random.RandomState(8).rand(len(e)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_export_and_catalogue_tables_are_encodes_cls_rows_and_within_the_row_measure(dtype):
    from pmgt_amd.datasets import MODE_INFERENCE, MCNSampler
    from pmgt_amd.evaluation import encode_catalogue, export_embeddings
    assert N_ITEMS % BATCH == 1                                       # the last batch is one sequence: below the fused kernel's Tseq >= 2
    S, seed, threads = 32, 29, 3
    cfg = po.default_cfg(**em.D256)
    params = em.randomise_layernorms(po.synth_params(cfg, 151), 152)
    tables = po.synth_tables(N_ITEMS, cfg["feat_hidden_sizes"], 9)
    smp = MCNSampler(catalogue_graph(), S - 1)
    eng = new_engine(cfg, params, tables, dtype)
    exported = export_embeddings(eng, smp, N_ITEMS, batch_size=BATCH, threads=threads, seed=seed)
    table = encode_catalogue(types.SimpleNamespace(engine=eng, item_num=N_ITEMS), smp, batch_size=BATCH, threads=threads, seed=seed)
    assert exported.dtype == np.float32 and table.dtype == torch.float32 and tuple(table.shape) == exported.shape == (N_ITEMS, 256)
    assert np.isfinite(exported).all()
    assert exported.tobytes() == table.cpu().numpy().tobytes()
    w = dict(cfg=cfg, params=params, tables=tables, probs=False, n=N_ITEMS, S=S)
    o64, y, ragged = [], [], []
    for lo in range(0, N_ITEMS, BATCH):
        tg = np.arange(2, N_ITEMS + 2)[lo: lo + BATCH]
        tgt = smp.batch(tg, MODE_INFERENCE, threads=threads, base_seed=seed, counter=lo)
        ids, mask = tgt["node_ids"].clone(), tgt["attention_mask"].clone()
        assert np.array_equal(ids[:, 0].numpy(), tg) and bool((mask[:, 0] == 1).all())
        ragged.append(float((mask == 0).float().mean()))
        last, _, _ = encode(eng, w, len(tg), hidden=False, ids=ids, mask=mask)
        assert launch_counts(("qkvc_attn_fwd",))["qkvc_attn_fwd"] == (0 if dtype == "fp32" or len(tg) < 2 else 2)
        assert last[:, 0].float().cpu().numpy().tobytes() == exported[lo: lo + len(tg)].tobytes(), lo
        o64.append(em.run_oracle(w, ids=ids, mask=mask)["cls"])
        if dtype == "fp32":
            y.append(em.run_oracle(w, ids=ids, mask=mask, dtype=torch.float32)["cls"])
        else:
            y.append(em.run_oracle(w, ids=ids, mask=mask, store=em.hook(cfg, em.by_node(w, len(tg))))["cls"])
    assert len(ragged) == 3 and all(0.2 < r < 0.8 for r in ragged), ragged
    rt = em.forward_ratios(dict(cls=exported), dict(cls=np.concatenate(o64)), dict(cls=np.concatenate(y)))
    print(f"encode measure drivers {dtype}: {em.worst(rt)}")
    assert set(rt) == {"cls:max", "cls:l2", "cls:row"} and not em.failing(rt), em.failing(rt)


# ---- negative controls ----------------------------------------------------------------------------------------------------------------------
def test_negative_control_a_truth_misstated_at_beta_053_fails_the_measure():
    w = em.world("probs")
    got = engine_quantities(*encode(engine("probs", "bf16"), w, w["T"]))
    o64, e16 = em.misstated_truth("probs")
    bad = em.failing(em.forward_ratios(got, o64, e16, w["mask"]))
    print(f"encode measure, negative control beta 0.53: {bad}")
    for l in range(w["cfg"]["num_hidden_layers"]):
        assert f"probs.{l}:max" in bad and f"probs.{l}:l2" in bad, bad


@pytest.mark.parametrize("n_seq", [3, 257])
def test_negative_control_a_sequence_with_its_neighbours_rows_fails_the_cls_row_kind(n_seq):
    w = em.world("tok")
    got = engine_quantities(*encode(engine("tok", "bf16"), w, n_seq))
    o64, e16 = em.yardstick("tok", n_seq, "bf16")
    assert not em.failing(em.forward_ratios(got, o64, e16))
    rt = em.forward_ratios(em.with_neighbours_rows(got, 1), o64, e16)
    print(f"encode measure, negative control mis-paired sequence of {n_seq}: cls max {rt['cls:max']:.1f} l2 {rt['cls:l2']:.1f} row {rt['cls:row']:.1f}")
    assert rt["cls:row"] > 10 * em.C_BOUND


# ---- 3. invariants --------------------------------------------------------------------------------------------------------------------------
INVARIANT_CASES = ("table_3", "token_3", "table_257", "token_257")
inv = lambda f: pytest.mark.parametrize("dtype", DTYPES)(pytest.mark.parametrize("label", INVARIANT_CASES)(f))


def inv_world(label):
    c = em.CASES[label]
    return em.world(c["world"]), c["T"]


def inv_engine(label, dtype):
    w, _ = inv_world(label)
    return new_engine(w["cfg"], w["params"], w["tables"], dtype)


def other_sequences(w, n_seq, seed):
    """n_seq further sequences on the world's graph"""
    return em.make_inputs(w["n"], n_seq, w["S"], seed)


@inv
def test_encode_is_repeatable_over_a_poisoned_workspace(label, dtype):
    """no read of a workspace byte the call did not write first: 0xFF bytes are a NaN in bf16 and in fp32"""
    w, n_seq = inv_world(label)
    eng = inv_engine(label, dtype)
    first = encode(eng, w, n_seq)
    ws = eng._workspace(int(eng.lib.pmgt_workspace_bytes(eng.h, n_seq, w["S"], 1, 0)))
    assert ws is eng._ws and ws.numel() > 0
    ws.fill_(0xFF)
    again = encode(eng, w, n_seq)
    assert eng._ws is ws
    for a, b in zip(first[:2], again[:2]):
        assert bool(torch.isfinite(b.float()).all()) and same_bits(a, b)
    # ... and on a workspace that was poisoned before the first call of an engine
    eng2 = inv_engine(label, dtype)
    eng2._workspace(ws.numel()).fill_(0xFF)
    fresh = encode(eng2, w, n_seq)
    for a, b in zip(first[:2], fresh[:2]):
        assert bool(torch.isfinite(b.float()).all()) and same_bits(a, b)


@inv
def test_encode_draws_nothing(label, dtype):
    from tests import bf16_measure_util as bm
    from tests.test_dropout_oracle_gpu import with_dropout
    _, n_seq = inv_world(label)
    case = with_dropout(bm.synth_case(n=2000, e=16000, cfgkw=em.D256, S=32, B=4, seed=91))
    assert case["cfg"]["hidden_dropout_prob"] > 0
    ids, mask = em.make_inputs(2000, n_seq, 32, 7)
    masked, _, _ = case["inj_cpu"]
    outs = []
    for encodes in (True, False):
        eng = new_engine(case["cfg"], case["params"], case["tables"], dtype)
        eng.rng_state[1] = 2
        before = eng.rng_state.clone()
        if encodes:
            eng.encode(ids=ids.cuda(), attention_mask=mask.cuda(), output_hidden_states=True)
            eng.encode(ids=ids.cuda(), attention_mask=mask.cuda(), output_attentions=True)
            torch.cuda.synchronize()
            assert torch.equal(eng.rng_state, before)
        out = eng.pretrain_step(dev_batch(case["batch"]), training=True, backward=True, nfr_inject=(masked.cuda(), case["full"].cuda()),
                                want_hidden=False)
        torch.cuda.synchronize()
        outs.append((out["losses"].clone(), out["logits"].clone(), eng.grads.clone()))
    for a, b in zip(*outs):
        assert bool(torch.isfinite(a).all()) and same_bits(a, b)


@inv
def test_encode_does_not_depend_on_the_order_or_the_company_of_a_sequence(label, dtype):
    w, n_seq = inv_world(label)
    eng = inv_engine(label, dtype)
    ids, mask = w["ids"][:n_seq], w["mask"][:n_seq]
    last, hs, _ = encode(eng, w, n_seq)
    perm = torch.randperm(n_seq, generator=torch.Generator().manual_seed(5))
    assert not torch.equal(perm, torch.arange(n_seq))
    last_p, hs_p, _ = encode(eng, w, n_seq, ids=ids[perm], mask=mask[perm])
    assert same_bits(last_p, last[perm.cuda()]) and same_bits(hs_p, hs[:, perm.cuda()])
    # sequence 0 at the end of a batch of other sequences (the ragged tile / the half-empty step), and in the middle
    for pos in (n_seq - 1, n_seq // 2):
        ids2, mask2 = other_sequences(w, n_seq, 77 + pos)
        ids2[pos], mask2[pos] = ids[0], mask[0]
        last2, hs2, _ = encode(eng, w, n_seq, ids=ids2, mask=mask2)
        assert same_bits(last2[pos], last[0]) and same_bits(hs2[:, pos], hs[:, 0]), pos


@inv
def test_node_ids_at_masked_positions_do_not_reach_a_valid_position(label, dtype):
    """a masked key has probability exactly 0 and adds exact zeros: what the shortcut layer and SURVEY Q6 rely on"""
    w, n_seq = inv_world(label)
    eng = inv_engine(label, dtype)
    ids, mask = w["ids"][:n_seq], w["mask"][:n_seq]
    last, hs, _ = encode(eng, w, n_seq)
    fill = torch.randint(2, w["n"] + 2, ids.shape, generator=torch.Generator().manual_seed(6))
    ids2 = torch.where(mask > 0, ids, fill)
    assert int((ids2 != ids).sum()) > 0
    last2, hs2, _ = encode(eng, w, n_seq, ids=ids2)
    valid = (mask > 0).cuda()
    assert same_bits(last2[valid], last[valid]) and same_bits(hs2[:, valid], hs[:, valid])
    assert not same_bits(hs2[0], hs[0])                               # the rows at the masked positions themselves did change


@inv
def test_the_outputs_of_encode_agree_with_each_other(label, dtype):
    w, n_seq = inv_world(label)
    eng = inv_engine(label, dtype)
    last, hs, pr = encode(eng, w, n_seq)
    L = w["cfg"]["num_hidden_layers"]
    assert pr is None and tuple(hs.shape) == (L + 1, n_seq, w["S"], 256)
    assert same_bits(hs[L], last)
    plain, none_hs, _ = encode(eng, w, n_seq, hidden=False)
    assert none_hs is None and same_bits(plain, last)

