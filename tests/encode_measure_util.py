"""The inference entry (Engine.encode) held to measured noise: inputs, references and the forward measure shared by
tests/test_encode_measure_cpu.py and tests/test_encode_measure_gpu.py.

THE MEASURE.  o64 = po.encoder_fwd in fp64 (want_hidden, want_probs where a case measures probabilities); the yardstick y is e16 for the
bf16 engine (the same call under bf16_measure_util.make_store, forward roundings only) and r32 for the fp32 engine (the oracle in float32
on the CPU, the convention of item_sim_util.case_ratio); C = dcn_util.C_BOUND; floor = 2^-22 max|o64| per quantity.
    max      max|x - o64|  <= C max(max|y - o64|, floor)                    last_hidden_state, hidden_states.0 .. L, cls, probs.0 .. L-1
    l2       ||x - o64||_2 <= C max(||y - o64||_2, floor sqrt(numel))       the same quantities
    row      cls = last[:, 0] as [n_seq, d] (what is exported): every sequence r
             ||(x - o64)[r]||_2 <= C max(||(y - o64)[r]||_2, median_r ||(y - o64)[r]||_2, floor sqrt(d))
    masked   probs.l with a mask: a key whose mask is 0 has probability == 0.0 in every row (ratio 0, or inf when one is not)
`forward_ratios` returns {quantity:kind -> error / yardstick}; a case passes when every ratio is <= C.

PROBABILITIES.  Every forward attention kernel writes `a.probs` from the fp32 registers BEFORE the probabilities are packed to bf16 for
P V (attention_mfma.hip: attn_fwd_mfma_kernel, attn_fwd_coop_kernel and attn_fwd_tiles_kernel store p, then pack_b / pack_col; attention.hip
never packs at all).  So e16's probabilities are the values the hook is handed at the "probs" site, taken before it rounds them
(`_KeepProbs`); what flows on into P V is rounded as everywhere else.

REFERENCES are computed once per world at its largest sequence count and sliced: a sequence's rows depend on no other sequence, so the
first n sequences of a reference are the reference of the first n sequences (floor, median and norms are taken over the slice)."""
import functools

import numpy as np
import torch

from oracle import pmgt_oracle as po
from tests import bf16_measure_util as bm
from tests.dcn_util import C_BOUND

D256 = bm.D256
D512 = bm.D512
D128 = dict(hidden_size=128, num_attention_heads=2, num_hidden_layers=1, intermediate_size=128)
I4D = dict(D256, intermediate_size=1024)
# the smallest sequence count whose 256-row tiles number 96 (gemm_nt_lnf_shape): 95 * 256 + 1 tokens of 32
I4D_TSEQ = -(-(95 * 256 + 1) // 32)

# name -> the model, the graph size, the largest sequence count a case takes from it, and what the references carry
#   n = 14: (n + 2) * 2 <= 32 tokens, table mode from one sequence on; n = 2 000: table mode from 126 sequences of 32 on;
#   n = 5 000: 2 (n + 2) = 10 004 tokens, token mode up to 312 sequences of 32
WORLDS = {
    "tab_small": dict(cfgkw=D256, S=32, n=14, T=3, seed=41),
    "tab": dict(cfgkw=D256, S=32, n=2000, T=258, seed=42),
    "tok": dict(cfgkw=D256, S=32, n=5000, T=258, seed=43),
    "nomask": dict(cfgkw=D256, S=32, n=5000, T=256, seed=44, mask=False),
    "beta_one": dict(cfgkw=D256, S=32, n=5000, T=256, seed=45, beta=1.0),
    "probs": dict(cfgkw=D256, S=32, n=5000, T=3, seed=46, probs=True),
    "d128_s65": dict(cfgkw=D128, S=65, n=5000, T=3, seed=47, probs=True),
    "d512": dict(cfgkw=D512, S=64, n=5000, T=65, seed=48),
    "i4d": dict(cfgkw=I4D, S=32, n=5000, T=I4D_TSEQ, seed=49),
}


def randomise_layernorms(params, seed):
    """gamma away from 1 and beta away from 0 in every LayerNorm (as tests/test_options_gpu.py does): a dropped gamma or beta shows"""
    g = torch.Generator().manual_seed(seed)
    out = dict(params)
    for k in sorted(params):
        if k.endswith("LayerNorm.weight"):
            out[k] = 0.7 + 0.6 * torch.rand(params[k].shape, generator=g)
        elif k.endswith("LayerNorm.bias"):
            out[k] = 0.2 * torch.randn(params[k].shape, generator=g)
    return out


def make_inputs(n, T, S, seed, masked=True):
    """ids [T, S] int64 (position 0: a node, distinct while the graph has enough) and a ragged 0/1 mask whose position 0 is always valid:
    sequence 0 is cut somewhere inside, sequence 1 keeps its CLS position alone, sequence 2 is full, the rest draw a length in 1 .. S.
    Masked positions carry the pad id 0, as the sampler writes them."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(2, n + 2, (T, S), generator=g)
    ids[:, 0] = (torch.randperm(n, generator=g)[:T] if n >= T else torch.randint(0, n, (T,), generator=g)) + 2
    if not masked:
        return ids, None
    lens = torch.randint(1, S + 1, (T,), generator=g)
    lens[0] = int(torch.randint(2, S, (1,), generator=g))
    if T > 1:
        lens[1] = 1
    if T > 2:
        lens[2] = S
    mask = (torch.arange(S)[None, :] < lens[:, None]).to(torch.float32)
    return torch.where(mask > 0, ids, torch.zeros_like(ids)), mask


@functools.lru_cache(maxsize=None)
def world(name):
    """cfg (dropout 0.1 in the config: inference must ignore it), parameters, tables and inputs of WORLDS[name]; computed once, never written"""
    spec = WORLDS[name]
    cfg = po.default_cfg(beta=spec.get("beta", 0.5), **spec["cfgkw"])
    assert cfg["hidden_dropout_prob"] == 0.1 and cfg["attention_probs_dropout_prob"] == 0.1
    params = randomise_layernorms(po.synth_params(cfg, spec["seed"] + 100), spec["seed"] + 200)
    tables = po.synth_tables(spec["n"], cfg["feat_hidden_sizes"], 9)
    ids, mask = make_inputs(spec["n"], spec["T"], spec["S"], spec["seed"], spec.get("mask", True))
    return dict(name=name, cfg=cfg, params=params, tables=tables, ids=ids, mask=mask, probs=spec.get("probs", False), n=spec["n"],
                T=spec["T"], S=spec["S"])


class _KeepProbs:
    """The hook with the probabilities kept as the engine reports them: before the rounding of the "probs" site (see the header)."""

    def __init__(self, inner):
        self.inner, self.probs = inner, []
        self.layer_norm = getattr(inner, "layer_norm", None)

    def __call__(self, x, name):
        if name.endswith(".probs"):
            self.probs.append(x.detach())
        return self.inner(x, name)


def quantities(last, hidden, probs):
    """the outputs of one forward -> {quantity: float64 numpy array}"""
    f = lambda t: np.asarray(t.detach().double().cpu().numpy())
    out = {"last_hidden_state": f(last), "cls": f(last[:, 0])}
    out.update({f"hidden_states.{i}": f(h) for i, h in enumerate(hidden)})
    if probs is not None:
        out.update({f"probs.{l}": f(p) for l, p in enumerate(probs)})
    return out


def run_oracle(w, ids=None, mask="own", dtype=torch.float64, store=None, autocast=False, cfg=None):
    """po.encoder_fwd on the world's inputs (or on ids / mask given) -> quantities.  autocast: the second bf16 realisation,
    torch.autocast("cpu", bfloat16) over fp32 parameters with the modality attention kept in fp32."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    ids = w["ids"] if ids is None else ids
    mask = w["mask"] if isinstance(mask, str) else mask
    cfg = w["cfg"] if cfg is None else cfg
    p = {k: v.to(dtype) for k, v in w["params"].items()}
    feats = po.gather_feats(ids, [t.to(dtype) for t in w["tables"]])
    keep = None
    if autocast:
        store = bm._Fp32ModalityAttention(len(cfg["feat_hidden_sizes"]), store)
    elif store is not None:
        store = keep = _KeepProbs(store)
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16, enabled=autocast):
        last, hidden, probs = po.encoder_fwd(p, cfg, feats, None if mask is None else mask.to(dtype), want_probs=w["probs"], want_hidden=True,
                                             store=store)
    if keep is not None and w["probs"]:
        probs = keep.probs
    return quantities(last, hidden, probs)


def hook(cfg, by_node):
    """the storage hook of the bf16 engine's forward; by_node: the per-node mixed row of the table mode exists and is rounded"""
    return bm.make_store(cfg, tokens=1 << 40 if by_node else 0, shortcut=False, n_nodes=1 if by_node else None)


@functools.lru_cache(maxsize=None)
def reference(name, kind):
    """kind: "o64", "r32", "e16" (token mode), "e16_node" (table mode), "ac" (the autocast realisation) -> quantities at the world's
    largest sequence count; computed once, shared, never written"""
    w = world(name)
    if kind == "o64":
        return run_oracle(w)
    if kind == "r32":
        return run_oracle(w, dtype=torch.float32)
    if kind == "ac":
        return run_oracle(w, dtype=torch.float32, autocast=True)
    assert kind in ("e16", "e16_node"), kind
    return run_oracle(w, store=hook(w["cfg"], kind == "e16_node"))


def take(q, n_seq):
    return {k: v[:n_seq] for k, v in q.items()}


def by_node(w, n_seq, by_ids=True):
    """`use_table_projection` of the engine for the first n_seq sequences of the world"""
    return by_ids and bm.table_mode(w["n"], len(w["cfg"]["feat_hidden_sizes"]), n_seq * w["S"])


def yardstick(name, n_seq, dtype, by_ids=True):
    """(o64, y) for the first n_seq sequences: y = e16 of the embedding mode the engine takes (bf16) or r32 (fp32)"""
    kind = "r32" if dtype == "fp32" else ("e16_node" if by_node(world(name), n_seq, by_ids) else "e16")
    return take(reference(name, "o64"), n_seq), take(reference(name, kind), n_seq)


# ---- the measure --------------------------------------------------------------------------------------------------------------------------
def forward_ratios(got, o64, e16, mask=None):
    """{quantity:kind -> error of `got` / yardstick}: see the header.  mask [n_seq, S] (0 / 1) adds the exact-zero check of masked keys."""
    out = {}
    for k, ref in o64.items():
        ref = np.asarray(ref, dtype=np.float64)
        x = np.asarray(got[k], dtype=np.float64).reshape(ref.shape)
        y = np.asarray(e16[k], dtype=np.float64).reshape(ref.shape)
        assert np.isfinite(x).all(), k
        floor = 2.0 ** -22 * float(np.abs(ref).max())
        dx, dy = x - ref, y - ref
        out[k + ":max"] = bm._ratio(np.abs(dx).max(), max(np.abs(dy).max(), floor))
        out[k + ":l2"] = bm._ratio(np.sqrt((dx ** 2).sum()), max(np.sqrt((dy ** 2).sum()), floor * np.sqrt(ref.size)))
        if k == "cls":
            rx, ry = np.sqrt((dx ** 2).sum(1)), np.sqrt((dy ** 2).sum(1))
            scale = np.maximum(np.maximum(ry, np.median(ry)), floor * np.sqrt(ref.shape[1]))
            out[k + ":row"] = float((rx / scale).max())
        if k.startswith("probs.") and mask is not None:
            dead = np.asarray(mask)[:, None, None, :] == 0                     # [n_seq, 1, 1, S]: the key axis
            out[k + ":masked"] = 0.0 if (x[np.broadcast_to(dead, x.shape)] == 0.0).all() else float("inf")
    return out


def worst(rt, n=3):
    return ", ".join(f"{k} {v:.2f}" for k, v in sorted(rt.items(), key=lambda kv: -kv[1])[:n])


def failing(rt):
    return {k: round(v, 2) for k, v in rt.items() if not v <= C_BOUND}


# ---- negative controls --------------------------------------------------------------------------------------------------------------------
BETA_WRONG = 0.53


@functools.lru_cache(maxsize=None)
def misstated_truth(name):
    """(o64, e16) of the world with beta mis-stated as 0.53 (token mode)"""
    w = world(name)
    cfg = dict(w["cfg"], beta=BETA_WRONG)
    return run_oracle(w, cfg=cfg), run_oracle(w, cfg=cfg, store=hook(cfg, False))


def with_neighbours_rows(got, r):
    """`got` with every row of sequence r overwritten by sequence r + 1's: a mis-paired sequence"""
    out = {k: np.array(v, copy=True) for k, v in got.items()}
    for v in out.values():
        v[r] = v[r + 1]
    return out


def kinds_failing(rt):
    """the kinds (max / l2 / row / masked) among the failing ratios"""
    return sorted({k.rsplit(":", 1)[1] for k in failing(rt)})


# ---- the cases (the CPU test and the GPU test run the same ones) ----------------------------------------------------------------------------
# label -> world, sequence count, entry ("ids" / "feats"), and for the bf16 engine the kernel families its launch trace must / must not hold
def _headline(n_seq, table):
    if n_seq == 1:                                   # 32 tokens: below the fused kernel's Tseq >= 2 and the streaming GEMMs' 64 rows
        expect, absent = ("nt_tile",), ("qkvc_attn_fwd", "gemm_ws", "gemm_wsr")
    elif n_seq * 32 < 8192:
        expect, absent = ("qkvc_attn_fwd", "gemm_ws"), ("gemm_wsr", "qkvc_attn_fwd_vc")
    else:
        expect, absent = ("qkvc_attn_fwd", "gemm_wsr"), ("qkvc_attn_fwd_vc",)
    return (expect + ("embed_tok8",), absent) if table else (expect, absent + ("embed_tok8",))


CASES = {}
for _T in (1, 2, 3, 255, 256, 257, 258):
    for _mode in ("table", "token"):
        _e, _a = _headline(_T, _mode == "table")
        CASES[f"{_mode}_{_T}"] = dict(world="tok" if _mode == "token" else ("tab_small" if _T <= 3 else "tab"), T=_T, table=_mode == "table",
                                      expect=_e, absent=_a)
CASES.update({
    "beta_one_256": dict(world="beta_one", T=256, expect=("qkvc_attn_fwd_vc", "gemm_wsr"), absent=("embed_tok8",)),
    "nomask_3": dict(world="nomask", T=3, expect=("qkvc_attn_fwd", "gemm_ws"), absent=("gemm_wsr", "embed_tok8")),
    "nomask_256": dict(world="nomask", T=256, expect=("qkvc_attn_fwd", "gemm_wsr"), absent=("embed_tok8",)),
    "feats_3": dict(world="tok", T=3, entry="feats", expect=("qkvc_attn_fwd", "gemm_ws"), absent=("gemm_wsr", "embed_tok8")),
    "feats_256": dict(world="tok", T=256, entry="feats", expect=("qkvc_attn_fwd", "gemm_wsr"), absent=("embed_tok8",)),
    "probs_3": dict(world="probs", T=3, expect=("gemm_ws",), absent=("qkvc_attn_fwd", "embed_tok8")),
    "d128_s65_probs": dict(world="d128_s65", T=3, expect=(), absent=("qkvc_attn_fwd", "attn_tiles_fwd", "embed_tok8")),
    "d512_64": dict(world="d512", T=64, expect=("gemm_rowln", "attn_tiles_fwd"), absent=("qkvc_attn_fwd", "embed_tok8")),
    "d512_65": dict(world="d512", T=65, expect=("gemm_rowln", "attn_tiles_fwd"), absent=("qkvc_attn_fwd", "embed_tok8")),
    "i4d": dict(world="i4d", T=I4D_TSEQ, table=True, expect=("nt_lnf", "qkvc_attn_fwd", "embed_tok8"), absent=()),
})


def case_truth(label, dtype="bf16"):
    """(world, n_seq, o64, yardstick, mask or None) of a case"""
    c = CASES[label]
    w = world(c["world"])
    by_ids = c.get("entry", "ids") == "ids"
    assert by_node(w, c["T"], by_ids) == c.get("table", False), label
    o64, y = yardstick(c["world"], c["T"], dtype, by_ids)
    return w, c["T"], o64, y, (None if w["mask"] is None else w["mask"][:c["T"]])
