"""The training step with dropout ON against the CPU oracle with the SAME masks.

Dropout in the kernels is a counter hash of (seed, step, site, row, column group); tests/dropout_util.py restates it bit for bit
(test_dropout_rng_gpu.py), so the oracle's `drop(x, name)` hook can apply exactly what the device draws:

  "emb"            site (-1, EMB)   row = token row m = seq * S + s of the concatenated step (targets, pairs, masked targets), col = channel
  <layer>...a1/a2  site (l, A1/A2)  row = (seq * H + head) * S + query, col = key
  <layer>ao / fo   site (l, AO/FO)  row = token row, col = channel -- except the last layer of the shortcut path (want_hidden = False), whose
                                    dense tail runs on compacted rows: the mask of token row need_rows[k] is row k of the site

An error the forward and backward kernels share (wrong site, mask after the residual, mixed probabilities dropped, a row index that differs
between the compacted forward and backward, a scale folded in twice) changes loss and gradients here by orders of magnitude more than the
bounds; the negative control at the end shows that by mis-stating the hook on the CPU side."""
import numpy as np
import pytest
import torch

from oracle import pmgt_oracle as po
from tests import dropout_util as du
from tests import golden_util as gu

pytestmark = pytest.mark.gpu

P_DROP = 0.1


def make_hook(cfg, seed, step, S, need=None, swap_sites=False, drop_mixed=False):
    """drop(x, name) for po.pretrain_forward.  need: compact row list of the last layer (shortcut path) or None."""
    L, H = cfg["num_hidden_layers"], cfg["num_attention_heads"]
    ph, pa = cfg["hidden_dropout_prob"], cfg["attention_probs_dropout_prob"]

    def mul(x, k, p):
        return x * torch.from_numpy(k).to(x.dtype).reshape(x.shape) * (1.0 / (1.0 - float(np.float32(p))))

    def drop(x, name):
        if name == "emb":
            T, S_, d = x.shape
            return mul(x, du.keep(seed, step, du.site_id(-1, du.SITE_EMB), T * S_, d, ph), ph)
        layer = int(name.split(".")[3])
        if name.endswith(".a1") or name.endswith(".a2"):
            kind = du.SITE_A1 if name.endswith(".a1") else du.SITE_A2
            if swap_sites:
                kind = du.SITE_A1 + du.SITE_A2 - kind
            T, H_, S_, _ = x.shape
            if drop_mixed:          # (mis-statement: one mask for both branches, as if the mixed probabilities were dropped)
                kind = du.SITE_A1
            return mul(x, du.keep(seed, step, du.site_id(layer, kind), T * H_ * S_, S_, pa), pa)
        kind = du.SITE_AO if name.endswith("ao") else du.SITE_FO
        assert name.endswith("ao") or name.endswith("fo"), name
        T, S_, d = x.shape
        site = du.site_id(layer, kind)
        if need is not None and layer == L - 1:
            k = np.ones((T * S_, d), dtype=bool)       # rows outside need_rows never reach the loss: any mask will do
            k[need] = du.keep(seed, step, site, len(need), d, ph)
        else:
            k = du.keep(seed, step, site, T * S_, d, ph)
        return mul(x, k, ph)
    return drop


def make_engine(case, dtype, options=()):
    from pmgt_amd.configuration_pmgt import PMGTConfig
    from pmgt_amd.engine import Engine
    cfg = {k: v for k, v in case["cfg"].items() if k != "fp8"}
    eng = Engine(PMGTConfig(**cfg), dtype=dtype, seed=0)
    for key in options:
        eng.set_option(key, 1)
    eng.load_params(case["params"])
    eng.set_tables(*[t.numpy() for t in case["tables"]])
    return eng


def dev_batch(batch):
    tgt, pair, num_pairs, labels = batch
    cu = lambda d: {k: v.cuda() for k, v in d.items()}
    return cu(tgt), cu(pair), num_pairs.cuda(), labels.cuda()


def with_dropout(case):
    case = dict(case)
    case["cfg"] = dict(case["cfg"], hidden_dropout_prob=P_DROP, attention_probs_dropout_prob=P_DROP)
    return case


def inject_from_full(full):
    """tgt_full [B, S] (-1 = not masked) -> the oracle's (m2 [B, S-1] bool, target ids in row-major order)."""
    m2 = full[:, 1:] >= 0
    return m2, full[:, 1:][m2]


def need_rows_of(batch, full):
    B, S = batch[0]["node_ids"].shape
    Pn = batch[1]["node_ids"].shape[0]
    b, s = np.nonzero(full.numpy() >= 0)
    return du.need_rows(B, Pn, S, (B + Pn + b) * S + s)


def run_oracle(case, inj_cpu, hook, dtype=torch.float64):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in case["params"].items()}
    tables = [t.to(dtype) for t in case["tables"]]
    ref = po.pretrain_forward(p, case["cfg"], tables, case["batch"], training=True, nfr_inject=inj_cpu, drop=hook)
    ref["loss"].backward()
    return p, ref


def fp32_excess(eng, out, p, ref):
    """max over everything compared of error / allowed error (<= 1 passes): loss, gsr, nfr rtol 1e-4; logits rtol 1e-4 (atol 1e-5);
    every named gradient rtol 2e-3 with atol 2e-3 of the tensor's RMS -- the fp32 bounds of tests/test_engine_gpu.py."""
    worst = {}
    for k in ("loss", "gsr", "nfr"):
        a, b = out[k].item(), ref[k].item()
        worst[k] = abs(a - b) / (1e-4 * abs(b))
    a, b = out["logits"].cpu().double().numpy(), ref["logits"].detach().double().numpy()
    worst["logits"] = float((np.abs(a - b) / (1e-5 + 1e-4 * np.abs(b))).max())
    for e in eng.entries:
        a = eng.view(e["name"], grad=True).detach().cpu().double().numpy()
        b = p[e["name"]].grad.double().numpy().reshape(a.shape)
        assert np.isfinite(a).all(), e["name"]
        rms = float(np.sqrt((b ** 2).mean()))
        worst["grad/" + e["name"]] = float((np.abs(a - b) / (2e-3 * rms + 1e-9 + 2e-3 * np.abs(b))).max())
    return worst


def golden_inject(case):
    ids = case["batch"][0]["node_ids"]
    masked, m2, tidx = gu.nfr_inject(case["gold"], ids, case["n_nodes"])
    full = torch.full_like(ids, -1)
    full[:, 1:][m2] = tidx
    return masked, m2, tidx, full


@pytest.mark.parametrize("want_hidden", [True, False])
@pytest.mark.parametrize("step", [0, 7])
@pytest.mark.parametrize("name", ["m1", "m1_pad", "m3", "m4", "e_script", "f3"])
def test_fp32_step_with_dropout_matches_the_oracle_with_restated_masks(name, step, want_hidden):
    """Golden cases (their batches, parameters, tables and NFR draws; only the dropout probabilities differ) at p = 0.1 on all five
    sites, step counter 0 and 7, full and shortcut (compact-row) last layer: loss, gsr, nfr, logits and every named gradient at the
    fp32 bounds.  Largest error / bound seen on MI355X: see the pull-request description (all below 0.2)."""
    case = with_dropout(gu.model_case(name))
    masked, m2, tidx, full = golden_inject(case)
    eng = make_engine(case, "fp32")
    eng.rng_state[1] = step
    seed, st = (int(v) for v in eng.rng_state.cpu())
    assert (seed, st) == (0, step)
    out = eng.pretrain_step(dev_batch(case["batch"]), training=True, backward=True, nfr_inject=(masked.cuda(), full.cuda()),
                            want_hidden=want_hidden)
    torch.cuda.synchronize()
    assert int(eng.rng_state[1]) == step + 1                     # the step advanced the counter: the next step draws fresh masks
    S = case["batch"][0]["node_ids"].shape[1]
    need = None if want_hidden else need_rows_of(case["batch"], full)
    p, ref = run_oracle(case, (masked, m2, tidx), make_hook(case["cfg"], seed, st, S, need))
    worst = fp32_excess(eng, out, p, ref)
    top = max(worst, key=worst.get)
    print(f"dropout-oracle fp32 {name} step={step} want_hidden={want_hidden}: worst error / bound = {worst[top]:.3f} ({top})")
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad
    assert int(out["nfr_count"].item()) == int(m2.sum())


def test_step_with_the_devices_own_nfr_masks_matches_the_oracle():
    """No injection (the path the benchmark runs): nfr_device_masks predicts the masked ids and targets nfr_generate draws from
    (seed, step); the oracle gets them as its injection.  Loss, nfr_count and gradients at the fp32 bounds, dropout on."""
    case = with_dropout(gu.model_case("m3"))
    ids = case["batch"][0]["node_ids"]
    for step, want_hidden in ((0, False), (3, True)):
        eng = make_engine(case, "fp32")
        eng.rng_state[1] = step
        out = eng.pretrain_step(dev_batch(case["batch"]), training=True, backward=True, want_hidden=want_hidden)
        torch.cuda.synchronize()
        wm, wt = du.nfr_device_masks(ids.numpy(), case["n_nodes"], 0, step, 0.02, 0.16)
        masked, full = torch.from_numpy(wm), torch.from_numpy(wt)
        m2, tidx = inject_from_full(full)
        assert int(out["nfr_count"].item()) == int(m2.sum()) > 0
        need = None if want_hidden else need_rows_of(case["batch"], full)
        p, ref = run_oracle(case, (masked, m2, tidx), make_hook(case["cfg"], 0, step, ids.shape[1], need))
        worst = fp32_excess(eng, out, p, ref)
        top = max(worst, key=worst.get)
        print(f"dropout-oracle device NFR masks step={step}: worst error / bound = {worst[top]:.3f} ({top})")
        assert all(v <= 1.0 for v in worst.values()), {k: v for k, v in worst.items() if not v <= 1.0}


@pytest.mark.parametrize("wrong", ["swap_sites", "drop_mixed", "full_rows_on_compact_path", "step_off_by_one"])
def test_negative_control_a_misstated_hook_fails_by_a_wide_margin(wrong):
    """The same comparison with the ORACLE's hook deliberately mis-stated (the engine run is an ordinary step): A1 / A2 sites swapped, one
    mask for both branches (= dropping the mixed probabilities), token-row masks on the compact-row path, the wrong step.  Each must
    miss the gradient bound by more than 10x: the test can see the class of error it exists for.  (The LOSS of this small model barely
    moves with the masks -- 0.2 to 11 times its bound on MI355X -- which is why every named gradient is compared, not the loss alone.)"""
    case = with_dropout(gu.model_case("m1"))
    masked, m2, tidx, full = golden_inject(case)
    eng = make_engine(case, "fp32")
    out = eng.pretrain_step(dev_batch(case["batch"]), training=True, backward=True, nfr_inject=(masked.cuda(), full.cuda()),
                            want_hidden=False)
    torch.cuda.synchronize()
    S = case["batch"][0]["node_ids"].shape[1]
    need = need_rows_of(case["batch"], full)
    kw = dict(swap_sites=wrong == "swap_sites", drop_mixed=wrong == "drop_mixed")
    hook = make_hook(case["cfg"], 0, 1 if wrong == "step_off_by_one" else 0, S, None if wrong == "full_rows_on_compact_path" else need, **kw)
    p, ref = run_oracle(case, (masked, m2, tidx), hook)
    worst = fp32_excess(eng, out, p, ref)
    grads = max(v for k, v in worst.items() if k.startswith("grad/"))
    print(f"negative control {wrong}: worst gradient error / bound = {grads:.1f}, loss error / bound = {worst['loss']:.1f}")
    assert grads > 10.0, (grads, worst["loss"])


# ---- bf16: the kernels the benchmark times ------------------------------------------------------------------------------------------------
def launch_counts(names):
    from pmgt_amd import _lib
    return {n: int(_lib.hip().pmgt_launch_trace_count(n.encode())) for n in names}


def bf16_compare(case, inj, full, expect, step=2, options=()):
    """bf16 engine (shortcut path, as the benchmark runs) against the fp32 oracle with restated masks: loss rtol 2e-2, per-tensor
    gradient cosine >= 0.99 -- the acceptance of tests/test_fullsize_oracle_gpu.py (`compare`, with its fp32-engine tie-breaker for
    cancellation-dominated bias sums; that engine draws the same masks)."""
    from pmgt_amd import _lib
    from tests.test_fullsize_oracle_gpu import compare
    masked, m2, tidx = inj
    S = case["batch"][0]["node_ids"].shape[1]

    def run(dtype):
        eng = make_engine(case, dtype, options)
        eng.rng_state[1] = step
        out = eng.pretrain_step(dev_batch(case["batch"]), training=True, backward=True, nfr_inject=(masked.cuda(), full.cuda()), want_hidden=False)
        torch.cuda.synchronize()
        return eng, out
    _lib.hip().pmgt_launch_trace_reset()
    eng, out = run("bf16")
    ran = launch_counts(list(expect))
    assert all(ran[k] >= 1 for k in expect), ran
    need = need_rows_of(case["batch"], full)
    p, ref = run_oracle(case, inj, make_hook(case["cfg"], 0, step, S, need), dtype=torch.float32)
    compare(eng, out, p, ref, "bf16", fp32_engine=lambda: run("fp32")[0])
    print(f"dropout-oracle bf16 {sorted(ran.items())}: loss {out['loss'].item():.5f} oracle {ref['loss'].item():.5f}")


def torch_inject(ids, n, seed):
    B, S = ids.shape
    g = torch.Generator().manual_seed(seed)
    r1, r2 = torch.rand(B, S - 1, generator=g), torch.rand(B, S - 1, generator=g)
    repl = torch.randint(2, n + 2, (B * (S - 1),), generator=g)
    masked, m2, tidx = po.nfr_masking(ids, n, r1, repl, r2)
    full = torch.full_like(ids, -1)
    full[:, 1:][m2] = tidx
    return (masked, m2, tidx), full


@pytest.mark.parametrize("beta", [0.5, 1.0])
def test_bf16_bench_shape_step_with_dropout_matches_the_oracle(beta):
    """Hidden 256 / 8 heads / S = 32 / L = 4 on the VG-sized graph, 96 targets drawn by the C++ sampler as curve_batches draws them: at least 8 192
    tokens and twice the table's rows, so the timed kernels are on the path (launch trace asserted); beta = 1 runs the vc forms."""
    from pmgt_amd.datasets import MODE_TRAIN, MCNSampler
    from pmgt_amd.graph import CSRGraph
    case = with_dropout(gu.curve_case("curve_c2"))
    case["cfg"]["beta"] = beta
    gold = case["gold"]
    n, edges, w = gu.graph(case["gname"])
    S, B = int(gold["S"]), 96
    smp = MCNSampler(CSRGraph.from_edge_list(n, edges, w), max_ctx_neigh=S - 1)       # as golden_util.curve_batches, with 96 targets
    smp.seed(int(gold["sseed"]))
    batch = smp.batch(gold["order"][:B] + 2, MODE_TRAIN, threads=0)
    case["batch"] = batch
    ids = batch[0]["node_ids"]
    tokens = (2 * ids.shape[0] + batch[1]["node_ids"].shape[0]) * ids.shape[1]
    assert tokens >= 8192 and tokens >= 2 * (n + 2), tokens          # streaming role-split GEMMs; the table-mode embedding (embed_tok8)
    inj, full = torch_inject(ids, case["n_nodes"], 5)
    expect = ["qkvc_attn_fwd", "attn_bwd_wgrad", "gemm_wsr", "gemm_wsr_lnb", "embed_tok8"] + (["attn_bwd_wgrad_vc2", "qkvc_attn_fwd_vc"] if beta == 1.0 else [])
    bf16_compare(case, inj, full, expect)


@pytest.mark.parametrize("shape", ["i4d", "d512_s64"])
def test_bf16_other_shapes_with_dropout_match_the_oracle(shape):
    """I = 4 d at d = 256 (the 256 x 256 tile with the LayerNorm forward / backward phases: nt_lnf, nt_lnb) and hidden 512 / S = 64 (the
    full-row LayerNorm tile gemm_rowln and the attention tile forms), each at the smallest batch that selects those kernels."""
    from tests.test_fullsize_oracle_gpu import make_case
    if shape == "i4d":
        cfgkw, S, B = dict(hidden_size=256, num_attention_heads=8, num_hidden_layers=2, intermediate_size=1024), 32, 72
        expect = ["nt_lnf", "nt_lnb", "qkvc_attn_fwd", "attn_bwd_wgrad"]
    else:
        cfgkw, S, B = dict(hidden_size=512, num_attention_heads=8, num_hidden_layers=2, intermediate_size=512), 64, 8
        expect = ["gemm_rowln", "attn_tiles_fwd", "attn_tiles_bwd"]
    base = make_case(7252, 88606, cfgkw, S=S, B=B, seed=31)
    case = with_dropout(dict(cfg=base["cfg"], params=base["params"], batch=base["batch"], n_nodes=7252,
                             tables=po.synth_tables(7252, base["cfg"]["feat_hidden_sizes"], 9)))
    masked, m2, tidx = base["inj_cpu"]
    full = base["inj"][1].cpu()
    ids = base["batch"][0]["node_ids"]
    tokens = (2 * ids.shape[0] + base["batch"][1]["node_ids"].shape[0]) * S
    assert tokens >= (96 * 256 - 255 if shape == "i4d" else 4096), tokens
    bf16_compare(case, (masked, m2, tidx), full, expect)
