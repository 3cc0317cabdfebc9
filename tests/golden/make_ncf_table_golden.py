"""Generates tests/golden/ncf_table_grad.npz: what the reference's own NCF gives, in fp64, when its item table is a trained parameter.
Imports the reference through `_ref_shim` (development container only, like make_ncf_train_golden.py); the fixture holds inputs and recorded
results.

  ncf_table_grad.npz  for model in (NeuMF-end, MLP): pmgt.ncf.models.NCF(5 users, 7 items, factor_num 8, num_layers 2) in fp64 with every
                      parameter perturbed from its init (the biases start at 0), 33 (user, item, label) pairs drawn from 4 users x 6 items
                      (duplicates are forced; user 4 and item 6 never appear), BCEWithLogitsLoss, backward: the weights under the project's
                      state_dict keys, the pairs, the loss, the logits and the gradient of every parameter, embed_item_MLP.weight -- the
                      item table -- included, under "item_table".
                          embed_user_MLP -> mlp_user_embeddings    embed_item_MLP -> the table    MLP_layers.{3 i} -> mlp_layers.{i}.linear
                          embed_*_GMF -> gmf_*_embeddings          predict_layer -> predict_layer
                      and a [9, 16] fp32 matrix with one zero row next to sklearn.preprocessing.normalize of it.  Its entries are seeded
                      multiples of 1/4 in [-2, 2]: the sum of 16 squares is then exact in fp32 in any order, the square root and the
                      quotient are correctly rounded, so the recorded bits hold on any machine.

Run: python tests/golden/make_ncf_table_golden.py
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
from sklearn.preprocessing import normalize  # noqa: E402

USER_NUM, ITEM_NUM, FACTOR, LAYERS, PAIRS = 5, 7, 8, 2, 33


def project_key(ref_key: str):
    """The reference's parameter name -> the project's state_dict key ("item_table" for the table)."""
    mod, leaf = ref_key.rsplit(".", 1)
    if mod == "embed_item_MLP":
        return "item_table"
    if mod == "embed_user_MLP":
        return "mlp_user_embeddings.weight"
    if mod in ("embed_user_GMF", "embed_item_GMF"):
        return f"gmf_{mod.split('_')[1]}_embeddings.weight"
    if mod.startswith("MLP_layers."):
        index = int(mod.split(".")[1])
        assert index % 3 == 0                                # Linear, Dropout, ReLU: no LayerNorm
        return f"mlp_layers.{index // 3}.linear.{leaf}"
    assert mod == "predict_layer"
    return ref_key


def table_grad_fixture(kind: str, seed: int) -> dict:
    torch.manual_seed(seed)
    model = NCF(USER_NUM, ITEM_NUM, factor_num=FACTOR, num_layers=LAYERS, emb_dropout=0.0, dropout=0.0, model=kind).double()
    gen = torch.Generator().manual_seed(seed + 1)
    used = {k: p for k, p in model.named_parameters() if kind != "MLP" or "GMF" not in k}
    with torch.no_grad():
        for p in used.values():                              # away from the init: biases are 0 and the embeddings 0.01 wide there
            p.add_(0.3 * torch.randn(p.shape, generator=gen, dtype=torch.float64))
    rng = np.random.default_rng(seed)
    users, items = rng.integers(0, USER_NUM - 1, size=PAIRS), rng.integers(0, ITEM_NUM - 1, size=PAIRS)
    labels = (rng.random(PAIRS) < 0.4).astype(np.float32)
    logits = model((torch.from_numpy(users), torch.from_numpy(items)))
    loss = torch.nn.BCEWithLogitsLoss()(logits, torch.from_numpy(labels).double())
    loss.backward()
    tag = "neumf" if kind == "NeuMF-end" else "mlp"
    out = {f"{tag}/users": users, f"{tag}/items": items, f"{tag}/labels": labels, f"{tag}/loss": np.float64(loss.item()),
           f"{tag}/logits": logits.detach().numpy()}
    for k, p in used.items():
        out[f"{tag}/w/{project_key(k)}"] = p.detach().numpy()
        out[f"{tag}/g/{project_key(k)}"] = p.grad.numpy()
    assert len(np.unique(users * ITEM_NUM + items)) < PAIRS and ITEM_NUM - 1 not in items and USER_NUM - 1 not in users
    print(f"ncf_table_grad: {kind}: loss {loss.item():.6f}, {len(used)} tensors")
    return out


def normalize_fixture() -> dict:
    rng = np.random.default_rng(11)
    x = (rng.integers(-8, 9, size=(9, 16)) / 4.0).astype(np.float32)
    x[4] = 0.0
    return {"norm/in": x, "norm/out": normalize(x.copy())}


if __name__ == "__main__":
    out = {}
    out.update(table_grad_fixture("NeuMF-end", 31))
    out.update(table_grad_fixture("MLP", 32))
    out.update(normalize_fixture())
    np.savez_compressed(os.path.join(HERE, "ncf_table_grad.npz"), **out)
