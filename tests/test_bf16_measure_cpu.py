"""The yardstick of the bf16 step measure (tests/bf16_measure_util.py), settled on the CPU without the code under test.

(a) HOOK OFF.  With store=None the oracle is the oracle from before the hook, bit for bit: the functions the hook was threaded through are
    kept below as they stood (`_before_*`), and loss, gsr, nfr, logits, last_hidden_state and every gradient of the m1 and m3 goldens are
    compared with `==` on their bytes; a hook that returns its argument changes nothing either.
(b) SECOND REALISATION.  The oracle under torch.autocast("cpu", bfloat16) with fp32 parameters -- another bf16 implementation, whose
    rounding points (every linear and matmul output, bf16 softmax inputs) are not the hook's -- must pass the measure against o64 / e16 on
    every quantity: a correct independent bf16 implementation has to pass what the engine has to pass.  Shapes: d = I = 256 / H 8 / S 32 /
    L 2 at 2 304 tokens (table mode, LayerNorm backward from the stored output in layer 0) and d = I = 512 / H 8 / S 64 / L 2 at 1 536
    tokens, each with dropout off and with dropout 0.1 through the restated masks, the same hook in all three runs.
    The one place where autocast leaves the contract both realisations restate is the modality attention of the embedding: the engine keeps
    its NF logits per node in fp32 registers, autocast would round them to bf16 (bf16_measure_util._Fp32ModalityAttention keeps that
    linear in fp32).  Largest ratio measured: d256 2.27, d256 + dropout 2.17, d512 2.50, d512 + dropout 2.66 -- each a weight-gradient row.
    The same realisation must also pass every synthetic step the GPU tests run, seed included (STEP_CASES: why a seed is part of a case).
(c) NEGATIVE CONTROLS.  Mis-statements of the model in the autocast run, the truth unchanged, each shifting the named gradient tensors by
    2 % to 10 % of their norm: today's acceptance (loss rtol 2e-2, per-tensor cosine >= 0.99) passes every one, the measure fails every
    one on the named tensors.  That pair of assertions is the gap this measure closes."""
import functools
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import pmgt_oracle as po
from tests import bf16_measure_util as bm
from tests import golden_util as gu
from tests.test_dropout_oracle_gpu import make_hook, need_rows_of, with_dropout

SHAPES = {
    "d256": dict(n=1000, e=8000, cfgkw=dict(hidden_size=256, num_attention_heads=8, num_hidden_layers=2, intermediate_size=256), S=32, B=6, seed=81),
    "d512": dict(n=1000, e=8000, cfgkw=dict(hidden_size=512, num_attention_heads=8, num_hidden_layers=2, intermediate_size=512), S=64, B=2, seed=82),
}
STEP = 2        # the dropout counter of the restated masks


# ---- (a) the oracle as it stood before the hook --------------------------------------------------------------------------------------------
def _before_embeddings_fwd(p, cfg, feats, drop=None):
    S = feats[0].shape[1]
    e = "bert.embeddings."
    fe = [po.linear_maybe_q(cfg, x, p[e + f"feat_linear.{i}.weight"], p[e + f"feat_linear.{i}.bias"], quant_x=False) for i, x in enumerate(feats)]
    z = F.linear(torch.tanh(torch.cat(fe, dim=-1)), p[e + "attention.1.weight"], p[e + "attention.1.bias"])
    a = torch.softmax(z, dim=-1)
    f = (a.unsqueeze(-1) * torch.stack(fe, dim=2)).sum(dim=2)
    pos = p[e + "position_embeddings.weight"][:S]
    role_ids = torch.ones(S, dtype=torch.long, device=f.device)
    role_ids[0] = 0
    role = p[e + "role_embeddings.weight"][role_ids]
    x = f + pos + role
    x = F.layer_norm(x, (x.shape[-1],), p[e + "LayerNorm.weight"], p[e + "LayerNorm.bias"], cfg["layer_norm_eps"])
    return drop(x, "emb") if drop is not None else x


def _before_self_attention_fwd(p, cfg, prefix, h, add_mask, drop=None):
    T, S, d = h.shape
    H = cfg["num_attention_heads"]
    dh = d // H
    beta = cfg["beta"]
    heads = lambda x: x.view(T, S, H, dh).permute(0, 2, 1, 3)
    q = heads(po.linear_maybe_q(cfg, h, p[prefix + "query.weight"], p[prefix + "query.bias"]))
    k = heads(po.linear_maybe_q(cfg, h, p[prefix + "key.weight"], p[prefix + "key.bias"]))
    v = heads(po.linear_maybe_q(cfg, h, p[prefix + "value.weight"], p[prefix + "value.bias"]))
    c = heads(po.linear_maybe_q(cfg, h, p[prefix + "ctx_attention.weight"], p[prefix + "ctx_attention.bias"]))
    rho = torch.linalg.norm(c, dim=-1, keepdim=True)
    rr = rho @ rho.transpose(-1, -2)
    eye = torch.eye(S, dtype=h.dtype, device=h.device)
    s1 = 1.0 - (c @ c.transpose(-1, -2)) / rr + eye + add_mask
    a1 = torch.softmax(s1, dim=-1)
    s2 = (q @ k.transpose(-1, -2)) / math.sqrt(dh) + add_mask
    a2 = torch.softmax(s2, dim=-1)
    if drop is not None:
        a1 = drop(a1, prefix + "a1")
        a2 = drop(a2, prefix + "a2")
    w = beta * a1 + (1.0 - beta) * a2
    return (w @ v).permute(0, 2, 1, 3).reshape(T, S, d)


def _before_layer_fwd(p, cfg, l, h, add_mask, drop=None):
    pre = f"bert.encoder.layer.{l}."
    eps = cfg["layer_norm_eps"]
    d = h.shape[-1]
    ctx = _before_self_attention_fwd(p, cfg, pre + "attention.self.", h, add_mask, drop)
    o = F.linear(ctx, p[pre + "attention.output.dense.weight"], p[pre + "attention.output.dense.bias"])
    if drop is not None:
        o = drop(o, pre + "ao")
    u = F.layer_norm(o + h, (d,), p[pre + "attention.output.LayerNorm.weight"], p[pre + "attention.output.LayerNorm.bias"], eps)
    g = po.gelu_erf(F.linear(u, p[pre + "intermediate.dense.weight"], p[pre + "intermediate.dense.bias"]))
    o2 = F.linear(g, p[pre + "output.dense.weight"], p[pre + "output.dense.bias"])
    if drop is not None:
        o2 = drop(o2, pre + "fo")
    return F.layer_norm(o2 + u, (d,), p[pre + "output.LayerNorm.weight"], p[pre + "output.LayerNorm.bias"], eps)


def _before_pretrain_forward(p, cfg, tables, batch, nfr_inject, drop=None):
    tgt, pair, num_pairs, labels = batch
    B, P = tgt["node_ids"].shape[0], pair["node_ids"].shape[0]
    masked_ids, m2, target_idx = nfr_inject
    ids = torch.cat([tgt["node_ids"], pair["node_ids"], masked_ids])
    msk = torch.cat([tgt["attention_mask"], pair["attention_mask"], tgt["attention_mask"]])
    feats = po.gather_feats(ids, tables)
    add_mask = (1.0 - msk.to(feats[0].dtype))[:, None, None, :] * -10000.0
    h = _before_embeddings_fwd(p, cfg, feats, drop)
    for l in range(cfg["num_hidden_layers"]):
        h = _before_layer_fwd(p, cfg, l, h, add_mask, drop)
    gsr, logits = po.gsr_loss(h[B:B + P][:, 0], h[:B][:, 0], num_pairs, labels)
    rows = h[B + P:][:, 1:][m2]
    losses = []
    for i, t in enumerate(po.gather_feats(target_idx, tables)):
        pred = F.linear(rows, p[f"nfr_loss.projections.{i}.weight"], p[f"nfr_loss.projections.{i}.bias"])
        losses.append(F.mse_loss(pred, t))
    nfr = torch.stack(losses).mean()
    return dict(loss=gsr + nfr, gsr=gsr, nfr=nfr, logits=logits, last_hidden_state=h[:B])


@pytest.mark.parametrize("name", ["m1", "m3"])
@pytest.mark.parametrize("dropout", [False, True])
def test_hook_off_is_the_oracle_from_before_the_hook_bit_for_bit(name, dropout):
    case = gu.model_case(name)
    if dropout:
        case = with_dropout(case)
    inj = gu.nfr_inject(case["gold"], case["batch"][0]["node_ids"], case["n_nodes"])
    drop = make_hook(case["cfg"], 0, STEP, case["batch"][0]["node_ids"].shape[1]) if dropout else None

    def run(fn):
        p = {k: v.clone().requires_grad_(True) for k, v in case["params"].items()}
        ref = fn(p)
        ref["loss"].backward()
        out = {k: ref[k].detach().numpy().tobytes() for k in ("loss", "gsr", "nfr", "logits", "last_hidden_state")}
        out.update({k: v.grad.numpy().tobytes() for k, v in p.items()})
        return out
    before = run(lambda p: _before_pretrain_forward(p, case["cfg"], case["tables"], case["batch"], inj, drop))
    off = run(lambda p: po.pretrain_forward(p, case["cfg"], case["tables"], case["batch"], training=True, nfr_inject=inj, drop=drop, store=None))
    same = run(lambda p: po.pretrain_forward(p, case["cfg"], case["tables"], case["batch"], training=True, nfr_inject=inj, drop=drop,
                                             store=lambda x, name: x))
    assert sorted(before) == sorted(off) == sorted(same)
    assert [k for k in before if before[k] != off[k]] == []
    assert [k for k in before if before[k] != same[k]] == []


def test_every_site_the_oracle_names_is_in_the_table_and_rounds_as_stated():
    case = gu.model_case("m1")
    inj = gu.nfr_inject(case["gold"], case["batch"][0]["node_ids"], case["n_nodes"])
    seen = set()

    def spy(x, name):
        seen.add(bm.site_of(name))
        return x
    po.pretrain_forward(dict(case["params"]), case["cfg"], case["tables"], case["batch"], training=True, nfr_inject=inj, store=spy)
    assert seen == set(bm.SITES), seen ^ set(bm.SITES)
    x = (torch.randn(7, 5, dtype=torch.float64) * 3).requires_grad_(True)
    g = torch.randn(7, 5, dtype=torch.float64)
    for mode in (bm.FWD, bm.BWD, bm.FWD | bm.BWD):
        y = bm._Round.apply(x, mode)
        (gx,) = torch.autograd.grad(y, x, g)
        assert torch.equal(y, bm.bf16_round(x) if mode & bm.FWD else x) and torch.equal(gx, bm.bf16_round(g) if mode & bm.BWD else g)
    # the LayerNorm that rebuilds x^ from its stored output: the plain LayerNorm's gradients up to the rounding of y
    w, b = (1 + 0.05 * torch.randn(5, dtype=torch.float64)).requires_grad_(True), (0.02 * torch.randn(5, dtype=torch.float64)).requires_grad_(True)
    gb = bm.bf16_round(g)
    got = torch.autograd.grad(bm._LnFromY.apply(x, w, b, 1e-12), (x, w, b), gb)
    want = torch.autograd.grad(F.layer_norm(x, (5,), w, b, 1e-12), (x, w, b), gb)
    for a, c in zip(got, want):
        assert float((a - c).abs().max()) <= 2.0 ** -6 * float(c.abs().max())


# ---- (b), (c): shared runs -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def world(shape, dropout):
    """case, its dropout hook, o64, e16 and the autocast run, computed once per (shape, dropout) and left unchanged"""
    case = bm.synth_case(**SHAPES[shape])
    drop = None
    if dropout:
        case = dict(with_dropout(case), full=case["full"], inj_cpu=case["inj_cpu"])
        drop = make_hook(case["cfg"], 0, STEP, SHAPES[shape]["S"], need_rows_of(case["batch"], case["full"]))
    store = bm.make_store(case["cfg"], bm.tokens_of(case), True, case["n_nodes"])
    o64 = bm.run_oracle(case, case["inj_cpu"], drop=drop)
    e16 = bm.run_oracle(case, case["inj_cpu"], drop=drop, store=store)
    ac = bm.run_oracle(case, case["inj_cpu"], dtype=torch.float32, drop=drop, autocast=True)
    return dict(case=case, drop=drop, o64=o64, e16=e16, ac=ac)


@pytest.mark.parametrize("dropout", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_an_independent_bf16_realisation_passes_the_measure(shape, dropout):
    w = world(shape, dropout)
    rt = bm.ratios(w["ac"], w["o64"], w["e16"])
    print(f"bf16 measure, autocast oracle {shape} dropout={dropout}: {len(rt)} ratios, worst {bm.worst(rt)}")
    assert len(rt) > 100 and not bm.failing(rt), bm.failing(rt)
    assert bm.old_acceptance(w["ac"], w["o64"]) == []
    # the yardstick itself is bf16 noise, not more: every gradient tensor of e16 within 3 % of its norm, 1 - cos below 5e-4
    for k, v in w["o64"].items():
        if k.startswith("grad/") and not k.endswith(".key.bias"):
            rel = np.linalg.norm(w["e16"][k] - v) / np.linalg.norm(v)
            assert rel < 3e-2, (k, rel)


@pytest.mark.parametrize("label", bm.CPU_CHECKED)
def test_the_yardstick_alone_accepts_the_steps_the_gpu_tests_run(label):
    """Every synthetic step of tests/test_bf16_step_measure_gpu.py (the two largest aside) with the second realisation in the engine's
    place: the case, seed included, is one a correct bf16 implementation passes (bf16_measure_util.STEP_CASES says why that is asked)."""
    w = bm.step_world(label)
    ac = bm.run_oracle(w["case"], w["case"]["inj_cpu"], dtype=torch.float32, drop=w["drop"], autocast=True, want_hidden=w["want_hidden"])
    rt = bm.ratios(ac, w["o64"], w["e16"])
    print(f"bf16 measure, autocast oracle on the GPU case {label}: worst {bm.worst(rt)}")
    assert not bm.failing(rt), bm.failing(rt)


@pytest.mark.parametrize("name,shortcut", [("m1", True), ("m1_pad", True), ("m3", True), ("f3", True), ("m1", False), ("m3", False)])
def test_the_yardstick_alone_accepts_the_golden_steps_the_gpu_tests_run(name, shortcut):
    """... and the golden cases: with the shortcut layer (test_bf16_step_measure_gpu) and with the full last layer
    (test_engine_gpu.test_bf16_mode_tracks_fp32)."""
    case = bm.golden_case(name)
    o64 = bm.run_oracle(case, case["inj_cpu"])
    e16 = bm.run_oracle(case, case["inj_cpu"], store=bm.make_store(case["cfg"], bm.tokens_of(case), shortcut, case["n_nodes"]))
    rt = bm.ratios(bm.run_oracle(case, case["inj_cpu"], dtype=torch.float32, autocast=True), o64, e16)
    print(f"bf16 measure, autocast oracle on the golden {name} shortcut={shortcut}: worst {bm.worst(rt)}")
    assert not bm.failing(rt), bm.failing(rt)


def _scaled(site, factor):
    return lambda x, name: x * factor if name.endswith(site) else x


L0 = "grad/bert.encoder.layer.0."
CONTROLS = {
    # name: (dropout, what the autocast run gets wrong, tensors it must shift by 2 .. 10 % and fail on)
    "beta_053": (False, dict(cfg_over=dict(beta=0.53)), [L0 + "attention.self.ctx_attention.weight", L0 + "attention.self.key.weight"]),
    "attn_out_dense_x103": (False, dict(store=_scaled("layer.0.ao.dense", 1.03)), [L0 + "attention.self.query.weight", L0 + "attention.self.value.weight"]),
    "ffn_out_dense_x105": (False, dict(store=_scaled("layer.0.fo.dense", 1.05)), [L0 + "intermediate.dense.weight", L0 + "output.dense.bias"]),
    "ao_dropout_scale_omitted": (True, dict(unscaled="bert.encoder.layer.1.ao"), ["grad/bert.encoder.layer.1.attention.self.value.weight",
                                                                               "grad/bert.encoder.layer.1.attention.self.query.weight"]),
}


@pytest.mark.parametrize("control", list(CONTROLS))
def test_negative_control_todays_acceptance_passes_what_the_measure_fails(control):
    dropout, wrong, named = CONTROLS[control]
    w = world("d256", dropout)
    case, drop = w["case"], w["drop"]
    cfg = dict(case["cfg"], **wrong.get("cfg_over", {}))
    if "unscaled" in wrong:      # the 1 / (1 - p) of one site left out
        keep = float(np.float32(1.0) - np.float32(case["cfg"]["hidden_dropout_prob"]))
        drop = lambda x, name, _d=drop: _d(x, name) * keep if name == wrong["unscaled"] else _d(x, name)
    bad = bm.run_oracle(case, case["inj_cpu"], dtype=torch.float32, drop=drop, autocast=True, cfg=cfg, store=wrong.get("store"))
    shift = {k: float(np.linalg.norm(bad[k] - w["o64"][k]) / np.linalg.norm(w["o64"][k])) for k in named}
    rt = bm.ratios(bad, w["o64"], w["e16"])
    print(f"negative control {control}: shifts {[round(v, 4) for v in shift.values()]}, worst {bm.worst(rt)}")
    assert all(0.02 <= v <= 0.10 for v in shift.values()), shift
    assert bm.old_acceptance(bad, w["o64"]) == []                          # today's acceptance lets it through
    failed = bm.failing(rt)
    for k in named:                                                         # the measure does not, on the tensors the error lives in
        assert any(f.startswith(k + ":") for f in failed), (k, failed)
