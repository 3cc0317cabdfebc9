"""The bf16 training step held to measured bf16 noise: the storage hook of the oracle and the project's measure on top of it.

THE HOOK.  `make_store(...)` returns the `store(x, name)` of oracle/pmgt_oracle.py: a straight-through rounding x.to(bfloat16).to(x.dtype)
on the way forward and the same rounding of the gradient on the way back, at the values the bf16 engine keeps in bf16.  SITES lists every
name with its directions; the engine line behind each is in DESIGN.md section 3.  Weights are rounded forward only (the GEMMs read the bf16
mirror, the weight gradient is an fp32 sum).  A LayerNorm whose input the engine does not keep takes x^ = (y - beta) / gamma from the
STORED output in its backward (`_LnFromY`); `ln_from_y_layers` restates the engine's decision.

THE MEASURE, with o64 = the oracle in fp64, e16 = the oracle in fp64 under the hook, x = the code under test, C = dcn_util.C_BOUND,
floor = 2^-22 max|o64|, per quantity (logits, last_hidden_state where given, every named gradient tensor):
    max      max|x - o64|   <= C max(max|e16 - o64|, floor)
    l2       ||x - o64||_2  <= C max(||e16 - o64||_2, floor sqrt(numel))
    row      (2-D gradients) every output row r:  ||(x - o64)[r]||_2 <= C max(||(e16 - o64)[r]||_2, median_r ||(e16 - o64)[r]||_2,
             floor sqrt(columns))
`ratios` returns {quantity:kind -> error / yardstick}; a case passes when every ratio is <= C.  Exactly-zero tensors (key.bias always;
query / key at beta = 1) have no noise to measure against and keep the bounds of test_fullsize_oracle_gpu.compare: |x| < 1e-4 of the
largest gradient element for key.bias, <= 1e-6 of it where the oracle reports exact zeros; their ratio is scaled so that C is that bound.
The scalars loss / gsr / nfr keep rtol 2e-2 (same scaling) and gsr gets |x - o64| <= C max|e16 logits - o64 logits|: BCE is 1-Lipschitz
in the logit and the GSR loss is a mean of means."""
import functools

import numpy as np
import torch

from oracle import pmgt_oracle as po
from tests.dcn_util import C_BOUND

FWD, BWD = 1, 2
# site (the name's last component) -> directions rounded
SITES = {
    "weight": FWD,           # the bf16 mirror of a GEMM weight; its gradient is an fp32 sum
    "emb.feat": FWD,         # feature-table rows in the engine dtype (frozen: no gradient)
    "emb.e": FWD | BWD,      # projected feature rows E / dE
    "emb.mix": FWD,          # table mode only: the per-node mixed row F_all (its gradient: fp32 segment sums)
    "emb.sum": FWD | BWD,    # mix + position + role as the embedding LayerNorm sees it / dF
    "emb.h0": FWD | BWD,     # h0 (after dropout) / d h0
    "qkvc": FWD | BWD,       # Q | K | V | C / dQ | dK | dV | dC
    "probs": FWD | BWD,      # mixed probabilities packed for P V / the score gradients packed for the key-side products
    "ctx": FWD | BWD,        # ctx / d ctx
    "ao.dense": BWD,         # gradient of the attention-output dense (the masked copy when dropout is on)
    "ao.sum": FWD | BWD,     # dropout(dense) + residual as LN1 sees it / the LayerNorm backward's dx
    "u": FWD | BWD,          # u / du
    "ff_pre": FWD | BWD,     # GELU pre-activation / its gradient
    "g": FWD,                # GELU activation (its gradient lives in the epilogue that multiplies by GELU')
    "fo.dense": BWD,
    "fo.sum": FWD | BWD,
    "out": FWD | BWD,        # layer output / its gradient (GSR writes d hL in bf16 too)
    "nfr.pred": FWD | BWD,   # NFR predictions / the scaled differences written over them
    "nfr.target": FWD,       # NFR targets: the same table rows
}


def bf16_round(x):
    return x.to(torch.bfloat16).to(x.dtype)


class _Round(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, mode):
        ctx.mode = mode
        return bf16_round(x) if mode & FWD else x.clone()

    @staticmethod
    def backward(ctx, g):
        return (bf16_round(g) if ctx.mode & BWD else g), None


class _LnFromY(torch.autograd.Function):
    """y = bf16(LayerNorm(x)); backward with x^ = (y - beta) / gamma from the stored y and the forward's rstd, dy rounded as stored."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        mean = x.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((x - mean) ** 2).mean(-1, keepdim=True) + eps)
        y = bf16_round((x - mean) * rstd * gamma + beta)
        ctx.save_for_backward(y, gamma, beta, rstd)
        return y

    @staticmethod
    def backward(ctx, dy):
        y, gamma, beta, rstd = ctx.saved_tensors
        dy = bf16_round(dy)
        xh = (y - beta) / gamma
        g = dy * gamma
        dx = (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True)) * rstd
        red = tuple(range(dy.dim() - 1))
        return dx, (dy * xh).sum(red), dy.sum(red), None


def site_of(name):
    for s in SITES:
        if name == s or name.endswith("." + s):
            return s
    raise KeyError(f"storage hook: no site for {name!r}")


def ln_from_y_layers(cfg, tokens, shortcut):
    """The layers whose two LayerNorm backwards rebuild x^ from the stored output: `ln_from_y_applies` of the engine (bf16, hidden 256, at
    least 64 rows, K = d and K = I powers of two >= 64, or I > 512 on the whole-row tile from 96 tiles of 256 rows on; never the compacted
    last layer of the shortcut path) -> (layers of LN1, layers of LN2)."""
    d, I, L = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"]
    full = range(L - 1 if shortcut else L)

    def applies(K):
        if d != 256:
            return False
        if K > 512:
            return K % 64 == 0 and tokens >= 4096 and -(-tokens // 256) >= 96
        return tokens >= 64 and K >= 64 and K & (K - 1) == 0
    return (set(full) if applies(d) else set()), (set(full) if applies(I) else set())


def table_mode(n_nodes, n_feats, tokens):
    """`use_table_projection` of the engine: the whole table is projected once and mixed per node."""
    return (n_nodes + 2) * max(2, n_feats) <= tokens


def make_store(cfg=None, tokens=0, shortcut=True, n_nodes=None):
    """store(x, name) for po.pretrain_forward.  cfg / tokens / shortcut / n_nodes select what depends on the engine's path: which
    LayerNorms take x^ from their output and whether the per-node mixed row exists (cfg = None: neither)."""
    ln1, ln2 = ln_from_y_layers(cfg, tokens, shortcut) if cfg is not None else (set(), set())
    by_node = cfg is not None and n_nodes is not None and table_mode(n_nodes, len(cfg["feat_hidden_sizes"]), tokens)

    def store(x, name):
        s = site_of(name)
        if s == "emb.mix" and not by_node:
            return x
        return _Round.apply(x, SITES[s])

    def layer_norm(x, w, b, eps, name):
        layer = int(name.split(".")[3])
        if layer in (ln1 if name.endswith(".u") else ln2):
            return _LnFromY.apply(x, w, b, eps)
        return store(torch.nn.functional.layer_norm(x, (x.shape[-1],), w, b, eps), name)
    store.layer_norm = layer_norm
    return store


class _Fp32ModalityAttention:
    """For the autocast realisation: the modality attention a = softmax(Wa tanh([e_0; e_1; ..]) + ba) and the mix sum_k a_k e_k in fp32.
    Autocast would run that linear in bf16 and round its NF logits per node; the engine's contract keeps them in fp32 registers
    (embed_mix_fwd_kernel reads the bf16 rows of E and does the rest in fp32), so a rounding there belongs to neither realisation of
    the contract -- and it alone moved d loss / d attention.1.bias (NF numbers that sum to zero) by 6 x the yardstick.
    Used as the `store` of an autocast run (no rounding of its own; `inner`: a further hook applied first): the region between the last
    "emb.e" and "emb.mix" runs with autocast off."""

    def __init__(self, n_feats, inner=None):
        self.nf, self.inner, self.seen, self.off = n_feats, inner, 0, None

    def __call__(self, x, name):
        if self.inner is not None:
            x = self.inner(x, name)
        if name == "emb.e":
            x = x.float()
            self.seen += 1
            if self.seen == self.nf:
                self.off = torch.autocast("cpu", enabled=False)
                self.off.__enter__()
        elif name == "emb.mix":
            self.off.__exit__(None, None, None)
            self.off, self.seen = None, 0
        return x


# ---- runs ---------------------------------------------------------------------------------------------------------------------------------
def run_oracle(case, inj_cpu, dtype=torch.float64, drop=None, store=None, cfg=None, autocast=False, want_hidden=False):
    """One training forward + backward of the oracle -> {quantity: float64 numpy array} (loss, gsr, nfr, logits, grad/<name>, and
    last_hidden_state when asked).  autocast: the second bf16 realisation, torch.autocast("cpu", bfloat16) over the oracle (fp32
    parameters), the modality attention kept in fp32 (`_Fp32ModalityAttention`); `store` is then a mis-statement hook or None."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    p = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in case["params"].items()}
    tables = [t.to(dtype) for t in case["tables"]]
    if autocast:
        store = _Fp32ModalityAttention(len(case["cfg"]["feat_hidden_sizes"]), store)
    with torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        ref = po.pretrain_forward(p, cfg if cfg is not None else case["cfg"], tables, case["batch"], training=True, nfr_inject=inj_cpu,
                                  drop=drop, store=store)
    ref["loss"].double().backward()
    out = {k: np.asarray(ref[k].detach().double().numpy()) for k in ("loss", "gsr", "nfr", "logits")}
    if want_hidden:
        out["last_hidden_state"] = ref["last_hidden_state"].detach().double().numpy()
    out.update({"grad/" + k: v.grad.double().numpy() for k, v in p.items()})
    return out


def engine_quantities(eng, out, want_hidden=False):
    got = {k: np.asarray(out[k].detach().double().cpu().numpy()) for k in ("loss", "gsr", "nfr", "logits")}
    if want_hidden:
        got["last_hidden_state"] = out["last_hidden_state"].detach().double().cpu().numpy()
    got.update({"grad/" + e["name"]: eng.view(e["name"], grad=True).detach().double().cpu().numpy() for e in eng.entries})
    return got


# ---- the measure --------------------------------------------------------------------------------------------------------------------------
def _ratio(err, scale):
    return float(err / scale) if scale > 0 else (0.0 if err == 0 else float("inf"))


def ratios(got, o64, e16):
    """{quantity:kind -> error of `got` / yardstick}: see the header."""
    out = {}
    gscale = max(float(np.abs(v).max()) for k, v in o64.items() if k.startswith("grad/"))
    for k, ref in o64.items():
        ref = np.asarray(ref, dtype=np.float64)
        x = np.asarray(got[k], dtype=np.float64).reshape(ref.shape)
        assert np.isfinite(x).all(), k
        if k in ("loss", "gsr", "nfr"):
            out[k + ":rtol"] = C_BOUND * _ratio(abs(float(x) - float(ref)), 2e-2 * abs(float(ref)))
            continue
        if k.endswith(".key.bias"):          # the softmax over keys is invariant to the key bias: exactly 0 in exact arithmetic
            assert float(np.abs(ref).max()) < 1e-4 * gscale, k
            out[k + ":zero"] = C_BOUND * float(np.abs(x).max()) / (1e-4 * gscale)
            continue
        if float(np.abs(ref).max()) == 0.0:  # a gradient the oracle reports as exactly zero (query / key at beta = 1)
            out[k + ":zero"] = C_BOUND * float(np.abs(x).max()) / (1e-6 * gscale)
            continue
        y = np.asarray(e16[k], dtype=np.float64).reshape(ref.shape)
        floor = 2.0 ** -22 * float(np.abs(ref).max())
        dx, dy = x - ref, y - ref
        out[k + ":max"] = _ratio(np.abs(dx).max(), max(np.abs(dy).max(), floor))
        out[k + ":l2"] = _ratio(np.sqrt((dx ** 2).sum()), max(np.sqrt((dy ** 2).sum()), floor * np.sqrt(ref.size)))
        if k.startswith("grad/") and ref.ndim == 2:
            rx, ry = np.sqrt((dx ** 2).sum(1)), np.sqrt((dy ** 2).sum(1))
            scale = np.maximum(np.maximum(ry, np.median(ry)), floor * np.sqrt(ref.shape[1]))
            out[k + ":row"] = float((rx / scale).max())
    dl = float(np.abs(np.asarray(e16["logits"], dtype=np.float64) - np.asarray(o64["logits"], dtype=np.float64)).max())
    floor = 2.0 ** -22 * float(np.abs(o64["logits"]).max())
    out["gsr:logits"] = _ratio(abs(float(got["gsr"]) - float(o64["gsr"])), max(dl, floor))
    return out


def worst(rt, n=4):
    top = sorted(rt.items(), key=lambda kv: -kv[1])[:n]
    return ", ".join(f"{k.replace('bert.encoder.layer.', 'L').replace('grad/', '')} {v:.2f}" for k, v in top)


def failing(rt):
    return {k: round(v, 2) for k, v in rt.items() if not v <= C_BOUND}


def old_acceptance(got, o64):
    """Today's bf16 acceptance without its fp32-engine tie-break: loss / gsr / nfr rtol 2e-2, logits atol 3e-2, per-tensor gradient cosine
    >= 0.99 (the zero tensors as in `ratios`), flat cosine > 0.999 -> the list of what it rejects (empty = accepted)."""
    bad = []
    for k in ("loss", "gsr", "nfr"):
        if not abs(float(got[k]) - float(o64[k])) <= 2e-2 * abs(float(o64[k])):
            bad.append(k)
    if not np.abs(np.asarray(got["logits"]) - np.asarray(o64["logits"])).max() <= 3e-2:
        bad.append("logits")
    names = [k for k in o64 if k.startswith("grad/")]
    gscale = max(float(np.abs(o64[k]).max()) for k in names)
    for k in names:
        a, b = np.asarray(got[k], dtype=np.float64).ravel(), np.asarray(o64[k], dtype=np.float64).ravel()
        if k.endswith(".key.bias") or float(np.abs(b).max()) == 0.0:
            if not float(np.abs(a).max()) < 1e-4 * gscale:
                bad.append(k)
            continue
        if not float(a @ b) / (np.linalg.norm(a) * np.linalg.norm(b)) >= 0.99:
            bad.append(k)
    fa, fb = np.concatenate([np.ravel(got[k]) for k in names]), np.concatenate([np.ravel(o64[k]) for k in names])
    if not float(fa @ fb) / (np.linalg.norm(fa) * np.linalg.norm(fb)) > 0.999:
        bad.append("flat")
    return bad


# ---- synthetic cases (the CPU tests and the GPU tests build the same ones) ----------------------------------------------------------------
def synth_case(n, e, cfgkw, S, B, seed, beta=0.5, regular=False):
    """A seeded step on a synthetic graph: batch from the host sampler, NFR draws from torch's generator, bf16-free fp32 parameters and
    tables -> dict(cfg, params, tables, batch, n_nodes, inj_cpu = (masked ids, mask, target ids), full = [B, S] targets or -1)."""
    from pmgt_amd.datasets import MODE_TRAIN, MCNSampler
    from pmgt_amd.graph import synthetic_graph, synthetic_graph_regular
    cfg = po.default_cfg(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, beta=beta, **cfgkw)
    graph = (synthetic_graph_regular if regular else synthetic_graph)(n, e, seed=seed)
    smp = MCNSampler(graph, max_ctx_neigh=S - 1)
    rs = np.random.RandomState(seed)
    targets = rs.choice(n, B, replace=False).astype(np.int64) + 2
    batch = smp.batch(targets, MODE_TRAIN, threads=4, base_seed=seed, counter=0)
    ids = batch[0]["node_ids"]
    g = torch.Generator().manual_seed(seed)
    r1, r2 = torch.rand(B, S - 1, generator=g), torch.rand(B, S - 1, generator=g)
    repl = torch.randint(2, n + 2, (B * (S - 1),), generator=g)
    masked, m2, tidx = po.nfr_masking(ids, n, r1, repl, r2)
    full = torch.full_like(ids, -1)
    full[:, 1:][m2] = tidx
    return dict(cfg=cfg, params=po.synth_params(cfg, seed + 1), tables=po.synth_tables(n, cfg["feat_hidden_sizes"], 9), batch=batch,
                n_nodes=n, inj_cpu=(masked, m2, tidx), full=full)


def golden_case(name):
    """A model case of tests/golden with its recorded NFR draws, in the layout of `synth_case`."""
    from tests import golden_util as gu
    case = gu.model_case(name)
    ids = case["batch"][0]["node_ids"]
    masked, m2, tidx = gu.nfr_inject(case["gold"], ids, case["n_nodes"])
    full = torch.full_like(ids, -1)
    full[:, 1:][m2] = tidx
    return dict(case, inj_cpu=(masked, m2, tidx), full=full)


def tokens_of(case):
    tgt, pair = case["batch"][0]["node_ids"], case["batch"][1]["node_ids"]
    return (2 * tgt.shape[0] + pair.shape[0]) * tgt.shape[1]


# ---- the synthetic steps of tests/test_bf16_step_measure_gpu.py --------------------------------------------------------------------------
# SEEDS.  d loss / d embeddings.attention.1.bias has NF elements that sum to zero (a softmax's logit gradient): with two modalities ONE
# number, a cancelling sum over all nodes whose size varies 100 x from batch to batch (7e-5 .. 9e-3 over six seeds of the streaming shape)
# while its rounding noise does not.  max|e16 - o64| of that tensor is then a single draw of the noise, not its scale: the quotient of two
# independent draws exceeds 4 once in six, for ANY correct implementation (seed 91 with the full last layer: e16 8.0e-5 of the tensor,
# the autocast realisation 8.3e-4).  The measure is left as it is; a step is admitted as a case when the yardstick ALONE accepts it: the
# second CPU realisation (run_oracle(autocast=True)) must pass the measure on every quantity of that very step.  That is decided on the
# CPU, never by the code under test: tests/test_bf16_measure_cpu.py asserts it for the golden cases and for every case below that it can
# afford (the two largest were checked once by hand with the same call: largest ratio 2.22 and 2.16).
D256 = dict(hidden_size=256, num_attention_heads=8, num_hidden_layers=2, intermediate_size=256)
D512 = dict(hidden_size=512, num_attention_heads=8, num_hidden_layers=2, intermediate_size=512)
STEP = 2        # the dropout counter the restated masks are drawn at
STEP_CASES = {
    "streaming": dict(n=2000, e=16000, cfgkw=D256, S=32, B=24, seed=91),
    "streaming_dropout": dict(n=2000, e=16000, cfgkw=D256, S=32, B=24, seed=91, dropout=True),
    "beta_one": dict(n=2000, e=16000, cfgkw=D256, S=32, B=24, seed=91, beta=1.0),
    "want_hidden": dict(n=2000, e=16000, cfgkw=D256, S=32, B=24, seed=93, want_hidden=True),
    "intermediate_4d": dict(n=7252, e=88606, cfgkw=dict(D256, intermediate_size=1024), S=32, B=72, seed=31),
    "hidden_512": dict(n=7252, e=88606, cfgkw=D512, S=64, B=8, seed=33),
    "tiles_256": dict(n=7252, e=88606, cfgkw=dict(D256, intermediate_size=1024), S=32, B=192, seed=21),
}
CPU_CHECKED = ("streaming", "streaming_dropout", "beta_one", "want_hidden", "hidden_512")


@functools.lru_cache(maxsize=None)
def step_world(label):
    """A case of STEP_CASES with its references, computed once and left unchanged -> dict(case, drop, want_hidden, dropout, o64, e16)."""
    from tests.test_dropout_oracle_gpu import make_hook, need_rows_of, with_dropout
    spec = dict(STEP_CASES[label])
    dropout, want_hidden = spec.pop("dropout", False), spec.pop("want_hidden", False)
    case = synth_case(**spec)
    drop = None
    if dropout:
        case = with_dropout(case)
        drop = make_hook(case["cfg"], 0, STEP, spec["S"], None if want_hidden else need_rows_of(case["batch"], case["full"]))
    store = make_store(case["cfg"], tokens_of(case), not want_hidden, case["n_nodes"])
    o64 = run_oracle(case, case["inj_cpu"], drop=drop, want_hidden=want_hidden)
    e16 = run_oracle(case, case["inj_cpu"], drop=drop, store=store, want_hidden=want_hidden)
    return dict(case=case, drop=drop, want_hidden=want_hidden, dropout=dropout, o64=o64, e16=e16)
