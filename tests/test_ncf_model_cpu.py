"""The stand-alone NCF model on the host, no GPU: the torch module ncf.NCF and the numpy yardstick ncf_model_grad_host against the
reference's own model in fp64 (tests/golden/ncf_model.npz, made by tests/golden/make_ncf_model_golden.py), the initialisation bit for bit,
the quirks of NeuMF-pre, the flat layout against ncf_head.py's and against the header, the decay rule, and every refusal.

Tolerance: fp64 against fp64 of the same formula in another order of sums: 1e-12 absolute on the loss, the logits and every gradient
(tests/test_dcn_head_cpu.py's)."""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.ncf import NCF
from pmgt_amd.ncf_head import head_layout, ncf_dropout_masks, table_layout
from pmgt_amd.ncf_model import (ITEM_MLP, check_ncf_model_covered, layer_keys, ncf_model_grad_host, ncf_model_layout, ncf_model_layout_slots,
                                ncf_model_shape)
from pmgt_amd.ncf_model_train import decays
from tests.ncf_model_util import GOLD, HEADS, NS, TAGS, fixture, head_id, ill_conditioned, torch_model, world


def build(tag, made=None, dtype=torch.float64):
    _, _, _, _, _, (factor, layers, kind, ln) = fixture(tag)
    extra = dict(GMF_model=made["gmf"], MLP_model=made["mlp_ln"], alpha=0.3) if kind == "NeuMF-pre" else {}
    return NCF(5, 7, factor_num=factor, num_layers=layers, use_layer_norm=ln, layer_norm_eps=1e-12, model=kind, **extra).to(dtype)


def loaded(tag):
    """The module holding the fixture's weights (for `pre`: built from fresh sub-models, every tensor then loaded strictly)."""
    w = fixture(tag)[0]
    made = {"gmf": build("gmf"), "mlp_ln": build("mlp_ln")} if tag == "pre" else None
    model = build(tag, made)
    assert list(model.state_dict().keys()) == [str(k) for k in GOLD[tag + "/keys"]]      # the keys AND their order
    assert all(tuple(v.shape) == w[k].shape for k, v in model.state_dict().items())
    model.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    return model.eval()


@pytest.mark.parametrize("tag", TAGS)
def test_the_module_loads_the_reference_state_dict_strictly_and_gives_its_gradients(tag):
    w, g, users, items, labels, _ = fixture(tag)
    model = loaded(tag)
    logits = model((torch.from_numpy(users), torch.from_numpy(items)))
    assert np.abs(logits.detach().numpy() - GOLD[tag + "/logits"]).max() <= 1e-12
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, torch.from_numpy(labels).double())
    loss.backward()
    assert abs(loss.item() - float(GOLD[tag + "/loss"])) <= 1e-12
    named = dict(model.named_parameters())
    assert sorted(k for k, p in named.items() if p.grad is None) == sorted(str(k) for k in GOLD[tag + "/nograd"])
    assert sorted(k for k, p in named.items() if p.grad is not None) == sorted(g)
    for k in g:
        assert np.abs(named[k].grad.numpy() - g[k]).max() <= 1e-12, k


def test_head_on_ready_item_rows_is_forward():
    for tag in ("neumf_ln", "gmf", "mlp_ln"):
        _, _, users, items, _, _ = fixture(tag)
        model = loaded(tag)
        u, i = torch.from_numpy(users), torch.from_numpy(items)
        assert torch.equal(model.head(u, i, model.embed_item_MLP(i)), model((u, i)))
    assert torch.equal(loaded("gmf").head(u, i, None), loaded("gmf")((u, i)))      # kind GMF ignores the rows


@pytest.mark.parametrize("tag", ("mlp_ln", "gmf", "pre"))
def test_the_initialisation_draws_what_the_reference_draws(tag):
    torch.manual_seed(5)
    made = {"gmf": build("gmf", dtype=torch.float32), "mlp_ln": build("mlp_ln", dtype=torch.float32)} if tag == "pre" else None
    sd = build(tag, made, dtype=torch.float32).state_dict()
    assert list(sd.keys()) == [str(k) for k in GOLD[f"init/{tag}/keys"]]
    for k, v in sd.items():
        ref = GOLD[f"init/{tag}/{k}"]
        assert v.dtype == torch.float32 and ref.dtype == np.float32 and np.array_equal(v.numpy(), ref), k


def test_neumf_pre_mixes_the_predict_layers_and_copies_only_the_linears():
    gmf, mlp = loaded("gmf").float(), loaded("mlp_ln").float()      # (fp32, the dtype the new model is constructed in: the copies are exact)
    assert mlp.predict_layer.bias.item() != 0
    pre = NCF(5, 7, 8, 2, use_layer_norm=True, model="NeuMF-pre", GMF_model=gmf, MLP_model=mlp, alpha=0.3)
    sd = pre.state_dict()
    assert any(k.startswith("GMF_model.") for k in sd) and any(k.startswith("MLP_model.") for k in sd)      # they are sub-modules
    # the reference zeroes every Linear bias of every sub-module BEFORE it copies: the pretrained biases are lost, in both places
    assert mlp.predict_layer.bias.item() == 0 and sd["predict_layer.bias"].item() == 0 and not sd["MLP_layers.0.bias"].any()
    assert torch.equal(sd["predict_layer.weight"], torch.cat([0.3 * gmf.predict_layer.weight, (1 - 0.3) * mlp.predict_layer.weight], dim=1).detach())
    for k in ("embed_user_GMF.weight", "embed_item_GMF.weight"):
        assert torch.equal(sd[k], gmf.state_dict()[k])
    for k in ("embed_user_MLP.weight", "embed_item_MLP.weight", "MLP_layers.0.weight", "MLP_layers.4.weight"):
        assert torch.equal(sd[k], mlp.state_dict()[k])
    for k in ("MLP_layers.2.weight", "MLP_layers.6.weight"):      # the LayerNorm gamma / beta are NOT copied
        assert (sd[k] == 1).all() and not (mlp.state_dict()[k] == 1).all()
    assert not sd["MLP_layers.2.bias"].any() and mlp.state_dict()["MLP_layers.2.bias"].any()
    built = {k[len("pre/built/"):]: GOLD[k] for k in GOLD.files if k.startswith("pre/built/")}      # the reference's own construction
    assert sorted(built) == sorted(sd) and np.array_equal(built["MLP_layers.2.weight"], np.ones(16)) and not built["predict_layer.bias"].any()


@pytest.mark.parametrize("tag", TAGS)
def test_the_numpy_yardstick_equals_the_reference_in_fp64(tag):
    w, g, users, items, labels, (factor, layers, kind, ln) = fixture(tag)
    assert ncf_model_shape(w, kind) == (factor, layers, kind, ln)
    loss, logits, grads = ncf_model_grad_host(w, users, items, labels, np.float64, kind=kind)
    assert abs(loss - float(GOLD[tag + "/loss"])) <= 1e-12 and np.abs(logits - GOLD[tag + "/logits"]).max() <= 1e-12
    assert sorted(grads) == sorted(g) == sorted(ncf_model_layout(factor, layers, kind, ln, 5, 7)[0])
    for k in g:
        assert grads[k].shape == g[k].shape and np.abs(grads[k] - g[k]).max() <= 1e-12, k
    for key, ids in (("embed_user_MLP.weight", users), ("embed_item_MLP.weight", items), ("embed_item_GMF.weight", items)):
        if key in grads:
            untouched = np.setdiff1d(np.arange(len(w[key])), ids)
            assert len(untouched) == 1 and not grads[key][untouched].any()
    frozen = ncf_model_grad_host(w, users, items, labels, np.float64, kind=kind, train_items=False)[2]
    assert sorted(frozen) == sorted(k for k in g if k != ITEM_MLP) and all(np.array_equal(frozen[k], grads[k]) for k in frozen)


@pytest.mark.parametrize("tag", ("neumf_ln", "gmf", "mlp_ln"))
def test_the_yardstick_under_masks_equals_the_module_with_the_masks_applied_by_hooks(tag):
    w, _, users, items, labels, (factor, layers, kind, ln) = fixture(tag)
    n = len(users)
    masks = ncf_dropout_masks(11, 3, n, factor, layers, "MLP" if kind == "MLP" else "NeuMF-end", 0.25, [0.2, 0.4])
    if kind == "GMF":
        masks = {"gmf": masks["gmf"]}                        # kind GMF draws the gmf site alone
    assert all(0 < keep.mean() < 1 for keep, _ in masks.values())
    loss, logits, grads = ncf_model_grad_host(w, users, items, labels, np.float64, kind=kind, masks=masks)
    model = loaded(tag)
    as_t = {k: torch.from_numpy(np.asarray(keep, dtype=np.float64) * np.float64(scale)) for k, (keep, scale) in masks.items()}
    # emb_dropout is called on the GMF product first, then on the concatenated input (the reference's order); kind GMF / MLP call it once
    order = [s for s in ("gmf", "emb") if s in as_t]
    calls = []
    model.emb_dropout.register_forward_hook(lambda mod, inp, out: (calls.append(1), out * as_t[order[len(calls) - 1]])[1])
    drops = [m for m in model.MLP_layers if isinstance(m, torch.nn.Dropout)]
    if kind != "GMF":
        for i, m in enumerate(drops):
            m.register_forward_hook(lambda mod, inp, out, i=i: out * as_t[f"layer{i}"])
    z = model((torch.from_numpy(users), torch.from_numpy(items)))
    ref = torch.nn.functional.binary_cross_entropy_with_logits(z, torch.from_numpy(labels).double())
    ref.backward()
    assert len(calls) == len(order)
    assert abs(loss - ref.item()) <= 1e-12 and np.abs(logits - z.detach().numpy()).max() <= 1e-12
    named = dict(model.named_parameters())
    for k, v in grads.items():
        assert np.abs(v - named[k].grad.numpy()).max() <= 1e-12, k


@pytest.mark.parametrize("kind", ("MLP", "NeuMF-end"))
@pytest.mark.parametrize("factor,layers", [(8, 1), (16, 3), (64, 3), (32, 4)])
def test_the_layout_without_layernorm_is_the_pmgt_ncf_heads(kind, factor, layers):
    key_map = {"embed_user_MLP.weight": "mlp_user_embeddings.weight", "embed_user_GMF.weight": "gmf_user_embeddings.weight",
               "embed_item_GMF.weight": "gmf_item_embeddings.weight", "predict_layer.weight": "predict_layer.weight",
               "predict_layer.bias": "predict_layer.bias", "embed_item_MLP.weight": "item_table"}
    for i in range(layers):
        key_map.update({f"MLP_layers.{3 * i}.{p}": f"mlp_layers.{i}.linear.{p}" for p in ("weight", "bias")})
    for train_items, theirs in ((True, table_layout), (False, head_layout)):
        mine, count = ncf_model_layout(factor, layers, kind, False, 11, 13, train_items)
        ref, ref_count = theirs(factor, layers, kind, 11, 13)
        assert count == ref_count and {key_map[k]: v for k, v in mine.items()} == ref
        assert [key_map[k] for k in mine] == list(ref)       # the same order


@pytest.mark.parametrize("h", HEADS, ids=head_id)
def test_the_layout_holds_what_the_kind_trains_at_aligned_offsets(h):
    factor, layers, kind, ln = h
    layout, count = ncf_model_layout(factor, layers, kind, ln, 11, 13)
    d = factor << (layers - 1)
    if kind == "GMF":
        assert list(layout) == ["embed_user_GMF.weight", "embed_item_GMF.weight", "predict_layer.weight", "predict_layer.bias"]
        assert layout["predict_layer.weight"][1] == (1, factor)
    else:
        for i in range(layers):
            keys = layer_keys(i, ln)
            assert [layout[k][1] for k in keys] == [(d >> i, 2 * (d >> i))] + [(d >> i,)] * 3
            offs = [layout[k][0] for k in keys]
            assert offs == sorted(offs) and offs[2] == offs[1] + (d >> i) and offs[3] == offs[2] + (d >> i)      # gamma then beta follow the bias
        assert list(layout)[-1] == ITEM_MLP and layout[ITEM_MLP][1] == (13, d)
    assert all(off % 8 == 0 for k, (off, _) in layout.items() if k != "predict_layer.bias")
    at = 0
    for k, (off, shape) in layout.items():
        assert at <= off < at + 8
        at = off + int(np.prod(shape))
    assert at == count
    slots = ncf_model_layout_slots(layout)
    assert len(slots) == _lib.NCF_MODEL_TENSORS and sorted(s for s in slots if s >= 0) == sorted(off for off, _ in layout.values())
    model_keys = list(NCF(11, 13, factor, layers, use_layer_norm=ln, model=kind).state_dict())
    assert set(layout) <= set(model_keys)


def test_the_header_declares_the_entries_and_the_constants_of_the_bindings():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "pmgt_capi.h")).read()
    for name in ("pmgt_ncf_model_layout", "pmgt_ncf_model_workspace_bytes", "pmgt_ncf_model_train_grad"):
        assert re.search(r"\b" + name + r"\(", text) and name in _lib.HIP_SYMBOLS
    for i, kind in enumerate(_lib.NCF_MODEL_KINDS):          # (the first two are #defines, the new ones enumerators)
        macro = "PMGT_NCF_" + kind.upper().replace("-", "_")
        assert int(re.search(r"\b" + macro + r"(?: =)? (\d+)", text).group(1)) == i
    assert int(re.search(r"PMGT_NCF_MODEL_TENSORS = (\d+)", text).group(1)) == _lib.NCF_MODEL_TENSORS
    fields = re.search(r"typedef struct pmgt_ncf_model \{(.*?)\} pmgt_ncf_model;", text, re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", fields, flags=re.S))
    assert names == [f[0] for f in _lib.NcfModelC._fields_]


@pytest.mark.parametrize("ln", (False, True))
@pytest.mark.parametrize("kind", _lib.NCF_MODEL_KINDS)
@pytest.mark.parametrize("factor,layers", [(8, 1), (8, 2), (16, 3), (32, 4)])
def test_the_library_lays_the_parameters_out_as_the_python_layout_does(factor, layers, kind, ln):
    lib = _lib.hip()                                         # (host code of the library: no GPU is touched)
    for train_items in (True, False):
        layout, count = ncf_model_layout(factor, layers, kind, ln, 11, 13, train_items)
        offs = (C.c_int64 * _lib.NCF_MODEL_TENSORS)()
        got = lib.pmgt_ncf_model_layout(factor, layers, _lib.NCF_MODEL_KINDS.index(kind), int(ln), int(train_items), 11, 13, offs)
        assert got == count and list(offs) == ncf_model_layout_slots(layout), (train_items, list(offs))


@pytest.mark.parametrize("tag", TAGS)
def test_the_decay_rule_names_the_reference_optimizers_decayed_group(tag):
    decayed = sorted(str(k) for k in GOLD[tag + "/decayed"])
    names = [k for k, _ in loaded(tag).named_parameters()]
    assert sorted(k for k in names if decays(k)) == decayed
    _, _, _, _, _, (factor, layers, kind, ln) = fixture(tag)
    if ln and kind != "GMF":
        assert decays("MLP_layers.2.weight") and not decays("MLP_layers.2.bias")      # the LayerNorm gammas DO decay, the betas do not


def test_every_refusal_names_its_limit():
    for args, text in [((12, 2, "MLP"), "factor_num = 12"), ((8, 0, "MLP"), "num_layers = 0"), ((8, 5, "NeuMF-end"), "num_layers = 5"),
                       ((64, 4, "MLP"), "= 512 above 256"), ((64, 4, "NeuMF-pre"), "above 256"), ((8, 2, "NeuMF"), "model kind 'NeuMF'"),
                       ((8, 2, "MLP", float("nan")), "layer_norm_eps"), ((8, 2, "MLP", -1e-5), "layer_norm_eps"),
                       ((8, 2, "MLP", float("inf")), "layer_norm_eps")]:
        with pytest.raises(ValueError, match=re.escape(text)):
            check_ncf_model_covered(*args)
    check_ncf_model_covered(64, 4, "GMF")                    # kind GMF reads no MLP tensor: d is not limited
    check_ncf_model_covered(64, 3, "NeuMF-pre", 0.0)
    with pytest.raises(ValueError, match="user_num"):
        ncf_model_layout(8, 2, "MLP", True, 0, 7)
    with pytest.raises(ValueError, match="item_num"):
        ncf_model_layout(8, 2, "MLP", True, 5, 2 ** 31)
    w, _, users, items, labels, _ = fixture("mlp_ln")
    with pytest.raises(ValueError, match="pass kind="):
        ncf_model_grad_host(w, users, items, labels)         # a whole state_dict with predict_layer [1, F]: MLP or GMF?
    with pytest.raises(ValueError, match=re.escape("users in [0, 5] outside [0, 5)")):
        ncf_model_grad_host(w, np.array([0, 5]), np.array([0, 1]), np.zeros(2, np.float32), kind="MLP")
    with pytest.raises(ValueError, match="model kind"):
        NCF(5, 7, model="NeuMF")


@pytest.mark.parametrize("h", HEADS, ids=head_id)
def test_the_pair_lists_are_well_conditioned_by_the_yardstick_alone(h):
    hw = world(h)                                            # (asserts the cap of 1 pair in 8 for every n of NS)
    assert not ill_conditioned(hw["w"], hw["kind"], hw["users"], hw["items"]).any()
    for n in NS:
        assert hw["redrawn"][:n].sum() * 8 <= n
    assert hw["users"].max() == 3 and hw["items"].max() == 5 and len(np.unique(hw["users"] * 7 + hw["items"])) < len(hw["users"])


def test_the_torch_realisation_of_a_seeded_model_equals_the_yardstick():
    hw = world(HEADS[1])
    n = 33
    model = torch_model(hw["w"], hw["shape"], torch.float64)
    z = model((torch.from_numpy(hw["users"][:n]), torch.from_numpy(hw["items"][:n])))
    _, logits, _ = ncf_model_grad_host(hw["w"], hw["users"][:n], hw["items"][:n], hw["labels"][:n], np.float64, layer_norm_eps=1e-12)
    assert np.abs(z.detach().numpy() - logits).max() <= 1e-12
