"""Generates tests/golden/dcn_grad.npz: what the reference's own Deep & Cross Network gives in fp64.  Imports the reference through
`_ref_shim` (development container only, like make_ncf_table_golden.py); the fixture holds inputs and recorded results.

  dcn_grad.npz  for tag, (factor_num, deep layers, cross layers, LayerNorm) in
                    ln     (8, 2, 3, on)        noln   (8, 2, 3, off)        run    (16, 1, 4, on), scripts/run_dcn.sh's shape:
                pmgt.dcn.models.DCN(5 users, 7 items, ...) in fp64 with every parameter perturbed from its init (for `noln` the
                embeddings are also scaled down, so that the cross net, which without LayerNorm multiplies x0 by (1 + s) per layer, keeps
                max |z| below 30), 33 (user, item, label) pairs drawn from 4 users x 6 items (duplicates are forced; user 4 and item 6
                never appear), BCEWithLogitsLoss, backward: the weights under the state_dict's own keys (the project's are the same),
                the pairs, the loss, the logits and the gradient of every parameter; "<tag>/nograd" lists the parameters whose .grad
                is None (the cross layers' unused `bias`), "<tag>/decayed" the names in the decayed group of the reference's optimizer.

The decayed group is taken from the reference's own get_optimizer (pmgt/base_trainer.py) when that module imports here; its imports
(optuna, pytorch_lightning, mlflow, ...) are heavier than the model's, and where one of them is missing the list is recorded from the rule
that function states instead -- no_decay = ["bias", "LayerNorm.weight"], a parameter decays unless its name contains one of the two -- and
"<tag>/decayed_from" says which of the two happened ("get_optimizer" or "rule").

Run: python tests/golden/make_dcn_golden.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _ref_shim  # noqa: E402

_ref_shim.install()

from pmgt.dcn.models import DCN  # noqa: E402  (reference)

USER_NUM, ITEM_NUM, PAIRS = 5, 7, 33
CASES = {"ln": (8, 2, 3, True, 41), "noln": (8, 2, 3, False, 42), "run": (16, 1, 4, True, 43)}


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


def fixture(tag: str) -> dict:
    factor, deep, cross, ln, seed = CASES[tag]
    torch.manual_seed(seed)
    model = DCN(USER_NUM, ITEM_NUM, factor_num=factor, deep_net_num_layers=deep, cross_net_num_layers=cross, emb_dropout=0.0, dropout=0.0,
                use_layer_norm=ln, layer_norm_eps=1e-12).double().eval()
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if not ln and "embeddings" in k:
                p.mul_(0.25)
            p.add_((0.3 if ln else 0.05) * torch.randn(p.shape, generator=gen, dtype=torch.float64))
    rng = np.random.default_rng(seed)
    users, items = rng.integers(0, USER_NUM - 1, size=PAIRS), rng.integers(0, ITEM_NUM - 1, size=PAIRS)
    labels = (rng.random(PAIRS) < 0.4).astype(np.float32)
    logits = model((torch.from_numpy(users), torch.from_numpy(items)))
    loss = torch.nn.BCEWithLogitsLoss()(logits, torch.from_numpy(labels).double())
    loss.backward()
    assert ln or float(logits.abs().max()) < 30
    assert len(np.unique(users * ITEM_NUM + items)) < PAIRS and ITEM_NUM - 1 not in items and USER_NUM - 1 not in users
    decayed, source = decayed_names(model)
    out = {f"{tag}/users": users, f"{tag}/items": items, f"{tag}/labels": labels, f"{tag}/loss": np.float64(loss.item()),
           f"{tag}/logits": logits.detach().numpy(), f"{tag}/shape": np.array([factor, deep, cross, int(ln)]),
           f"{tag}/nograd": np.array([k for k, p in model.named_parameters() if p.grad is None]),
           f"{tag}/decayed": np.array(decayed), f"{tag}/decayed_from": np.array(source)}
    for k, p in model.named_parameters():
        out[f"{tag}/w/{k}"] = p.detach().numpy()
        if p.grad is not None:
            out[f"{tag}/g/{k}"] = p.grad.numpy()
    print(f"dcn_grad: {tag}: loss {loss.item():.6f}, max |z| {float(logits.abs().max()):.3f}, nograd {list(out[f'{tag}/nograd'])}, "
          f"decayed from {source}")
    return out


if __name__ == "__main__":
    out = {}
    for tag in CASES:
        out.update(fixture(tag))
    np.savez_compressed(os.path.join(HERE, "dcn_grad.npz"), **out)
