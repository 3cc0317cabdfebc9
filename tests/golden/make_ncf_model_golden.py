"""Generates tests/golden/ncf_model.npz: what the reference's own stand-alone NCF model gives in fp64.  Imports the reference through
`_ref_shim` (development container only, like make_dcn_golden.py); the fixture holds inputs and recorded results.

  ncf_model.npz  for tag, (factor_num, num_layers, kind, LayerNorm) in
                     mlp_ln (8, 2, MLP, on)   neumf_ln (8, 2, NeuMF-end, on)   gmf (8, 2, GMF, -)   neumf_noln (16, 3, NeuMF-end, off)
                     pre    (8, 2, NeuMF-pre, on), built from the `gmf` and `mlp_ln` models with alpha 0.3:
                 pmgt.ncf.models.NCF(5 users, 7 items, ...) in fp64 with every parameter perturbed from its init, 33 (user, item, label)
                 pairs drawn from 4 users x 6 items (duplicates are forced; user 4 and item 6 never appear), BCEWithLogitsLoss, backward:
                 the weights under the state_dict's own keys, the pairs, the loss, the logits and the gradient of every parameter that has
                 one; "<tag>/keys" the state_dict's keys in order, "<tag>/nograd" the parameters whose .grad is None, "<tag>/decayed" the
                 names in the decayed group of the reference's optimizer.  `pre` is constructed from the PERTURBED gmf and mlp_ln models
                 and is then perturbed itself; "pre/built/<key>" holds its state_dict right after construction.
                 "init/<tag>/<key>" for mlp_ln, gmf and pre: the freshly initialised fp32 state_dict after torch.manual_seed(5) (for
                 `pre`: manual_seed(5), then a GMF, an MLP model with LayerNorm and the NeuMF-pre are constructed in that order).

The decayed group is taken from the reference's own get_optimizer (pmgt/base_trainer.py) when that module imports here; where one of its
imports is missing the list is recorded from the rule that function states instead -- no_decay = ["bias", "LayerNorm.weight"], a parameter
decays unless its name contains one of the two -- and "<tag>/decayed_from" says which of the two happened ("get_optimizer" or "rule").

Run: python tests/golden/make_ncf_model_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_shim  # noqa: E402

_ref_shim.install()

from pmgt.ncf.models import NCF  # noqa: E402  (reference)

USER_NUM, ITEM_NUM, PAIRS = 5, 7, 33
CASES = {"mlp_ln": (8, 2, "MLP", True, 51), "neumf_ln": (8, 2, "NeuMF-end", True, 52), "gmf": (8, 2, "GMF", False, 53),
         "neumf_noln": (16, 3, "NeuMF-end", False, 54), "pre": (8, 2, "NeuMF-pre", True, 55)}
ALPHA = 0.3


def decayed_names(model):
    try:
        from pmgt.base_trainer import get_optimizer  # (reference)

        class Args(dict):
            __getattr__ = dict.__getitem__

        optim = get_optimizer(Args(model=model, decay=0.01, lr=1e-3, optim="sgd"))
        ids = {id(p) for p in optim.param_groups[0]["params"]}
        return [n for n, p in model.named_parameters() if id(p) in ids], "get_optimizer"
    except ImportError:
        no_decay = ["bias", "LayerNorm.weight"]
        return [n for n, _ in model.named_parameters() if not any(nd in n for nd in no_decay)], "rule"


def build(tag: str, made: dict):
    factor, layers, kind, ln, _ = CASES[tag]
    extra = dict(GMF_model=made["gmf"], MLP_model=made["mlp_ln"], alpha=ALPHA) if kind == "NeuMF-pre" else {}
    return NCF(USER_NUM, ITEM_NUM, factor_num=factor, num_layers=layers, emb_dropout=0.0, dropout=0.0, use_layer_norm=ln, layer_norm_eps=1e-12,
               model=kind, **extra)


def fixture(tag: str, made: dict) -> dict:
    factor, layers, kind, ln, seed = CASES[tag]
    torch.manual_seed(seed)
    model = build(tag, made).double().eval()
    out = {}
    if kind == "NeuMF-pre":
        out.update({f"{tag}/built/{k}": v.detach().numpy().copy() for k, v in model.state_dict().items()})
    gen = torch.Generator().manual_seed(seed + 1)
    own = [(k, p) for k, p in model.named_parameters() if not k.startswith(("GMF_model.", "MLP_model."))]
    with torch.no_grad():
        for k, p in own:
            p.add_((0.3 if "MLP_layers" in k or "predict" in k else 0.5) * torch.randn(p.shape, generator=gen, dtype=torch.float64))
    made[tag] = model
    rng = np.random.default_rng(seed)
    users, items = rng.integers(0, USER_NUM - 1, size=PAIRS), rng.integers(0, ITEM_NUM - 1, size=PAIRS)
    labels = (rng.random(PAIRS) < 0.4).astype(np.float32)
    model.zero_grad()
    logits = model((torch.from_numpy(users), torch.from_numpy(items)))
    loss = torch.nn.BCEWithLogitsLoss()(logits, torch.from_numpy(labels).double())
    loss.backward()
    assert float(logits.detach().abs().max()) < 30
    assert len(np.unique(users * ITEM_NUM + items)) < PAIRS and ITEM_NUM - 1 not in items and USER_NUM - 1 not in users
    decayed, source = decayed_names(model)
    out.update({f"{tag}/users": users, f"{tag}/items": items, f"{tag}/labels": labels, f"{tag}/loss": np.float64(loss.item()),
                f"{tag}/logits": logits.detach().numpy(), f"{tag}/shape": np.array([factor, layers, int(ln)]), f"{tag}/kind": np.array(kind),
                f"{tag}/keys": np.array(list(model.state_dict().keys())),
                f"{tag}/nograd": np.array([k for k, p in model.named_parameters() if p.grad is None]),
                f"{tag}/decayed": np.array(decayed), f"{tag}/decayed_from": np.array(source)})
    for k, v in model.state_dict().items():
        out[f"{tag}/w/{k}"] = v.detach().numpy().copy()
    for k, p in model.named_parameters():
        if p.grad is not None:
            out[f"{tag}/g/{k}"] = p.grad.numpy().copy()
    print(f"ncf_model: {tag}: loss {loss.item():.6f}, max |z| {float(logits.detach().abs().max()):.3f}, {len(out[f'{tag}/nograd'])} without grad, "
          f"decayed from {source}")
    return out


def fresh() -> dict:
    out = {}
    for tag in ("mlp_ln", "gmf", "pre"):
        torch.manual_seed(5)
        made = {}
        if tag == "pre":
            made["gmf"] = build("gmf", made)
            made["mlp_ln"] = build("mlp_ln", made)
        model = build(tag, made)
        out.update({f"init/{tag}/{k}": v.detach().numpy().copy() for k, v in model.state_dict().items()})
        out[f"init/{tag}/keys"] = np.array(list(model.state_dict().keys()))
    return out


if __name__ == "__main__":
    out, made = {}, {}
    for tag in ("mlp_ln", "neumf_ln", "gmf", "neumf_noln", "pre"):
        out.update(fixture(tag, made))
    out.update(fresh())
    np.savez_compressed(os.path.join(HERE, "ncf_model.npz"), **out)
