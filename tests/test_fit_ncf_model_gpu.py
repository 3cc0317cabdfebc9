"""fit_ncf_model on a planted set of 40 users x 30 items (user u likes the items i with (u + i) % 3 == 0: ten each; seven are training
pairs, one is the held-out positive among twelve candidates): three epochs with LayerNorm on, the history's keys, the best epoch restored
and kept as a file that a fresh NCF loads strictly, evaluate_ranking on the NCF, the NeuMF-pre built from a trained GMF and a trained MLP
model, and item_init."""
import glob
import os

import numpy as np
import pytest
import torch

from pmgt_amd import fit_ncf_model
from pmgt_amd.evaluation import evaluate_ranking
from pmgt_amd.metrics import RankingMetrics
from pmgt_amd.ncf import NCF

pytestmark = pytest.mark.gpu

USERS, ITEMS, CANDS = 40, 30, 12
SETTINGS = dict(batch_size=64, num_ng=4, seed=3, lr=1e-2, max_grad_norm=5.0)
KEYS = ["epoch", "train_loss", "n10", "n20", "r10", "r20", "loss", "best"]      # fit_ncf's row


def planted():
    rng = np.random.default_rng(17)
    pairs, cand, labels = [], np.zeros((USERS, CANDS), np.int64), np.zeros((USERS, CANDS), np.float32)
    for u in range(USERS):
        liked = np.array([i for i in range(ITEMS) if (u + i) % 3 == 0])
        other = np.array([i for i in range(ITEMS) if (u + i) % 3 != 0])
        rng.shuffle(liked)
        pairs += [(u, int(i)) for i in liked[:7]]
        cand[u] = np.concatenate([liked[7:8], rng.choice(other, CANDS - 1, replace=False)])
        labels[u, 0] = 1.0
    return np.array(pairs), (np.arange(USERS, dtype=np.int64), cand, labels, np.full(USERS, CANDS, np.int32))


def model_of(kind, seed=1, **kw):
    torch.manual_seed(seed)
    return NCF(USERS, ITEMS, factor_num=8, num_layers=2, use_layer_norm=True, model=kind, **kw).cuda()


def test_three_epochs_keep_and_restore_the_best_and_the_file_loads_strictly(tmp_path):
    pairs, valid = planted()
    model = model_of("NeuMF-end")
    history = fit_ncf_model(model, pairs, valid, max_epochs=3, early_criterion="loss", patience=3, ckpt_dir=str(tmp_path), **SETTINGS)
    assert len(history) == 3 and all(list(h) == KEYS for h in history)
    assert all(np.isfinite(h[k]) for h in history for k in KEYS[1:7]) and history[-1]["train_loss"] < history[0]["train_loss"]
    print("train_loss " + " ".join(f"{h['train_loss']:.4f}" for h in history) + "; validation loss " + " ".join(f"{h['loss']:.4f}" for h in history))
    best = max((h for h in history if h["best"]), key=lambda h: h["epoch"])
    files = glob.glob(os.path.join(str(tmp_path), "*.ckpt"))
    assert len(files) == 1 and f"epoch={best['epoch']:02d}" in os.path.basename(files[0])
    ckpt = torch.load(files[0], weights_only=False)
    assert ckpt["epoch"] == best["epoch"] and ckpt["metrics"] == best
    now = model.state_dict()                                 # the best epoch's parameters are back in the model
    assert list(ckpt["state_dict"]) == list(now) and all(torch.equal(now[k].cpu(), ckpt["state_dict"][k]) for k in now)
    fresh = model_of("NeuMF-end", seed=2)
    fresh.load_state_dict(ckpt["state_dict"], strict=True)
    # evaluate_ranking on the NCF: the device from its parameters, the table its own embed_item_MLP; the best epoch's validation row
    for m in (model, fresh):
        res = evaluate_ranking(m, None, *valid, metrics="device")
        assert all(abs(res[k] - best[k]) <= 1e-9 for k in ("n10", "n20", "r10", "r20")) and abs(res["loss"] - best["loss"]) <= 1e-6
    host = evaluate_ranking(model, None, *valid, metrics="host", table=model.embed_item_MLP.weight.detach())
    assert all(abs(host[k] - best[k]) <= 1e-9 for k in ("n10", "n20", "r10", "r20"))
    with pytest.raises(ValueError, match="table"):
        evaluate_ranking(model, None, *valid, table=model.embed_item_MLP.weight.detach()[:-1])


def test_a_trained_gmf_and_a_trained_mlp_model_build_a_neumf_pre():
    pairs, valid = planted()
    gmf, mlp = model_of("GMF"), model_of("MLP", seed=2)
    for m in (gmf, mlp):
        history = fit_ncf_model(m, pairs, valid, max_epochs=3, **SETTINGS)
        assert len(history) == 3 and history[-1]["train_loss"] < history[0]["train_loss"]
    alpha = 0.3
    pre = NCF(USERS, ITEMS, 8, 2, use_layer_norm=True, model="NeuMF-pre", GMF_model=gmf, MLP_model=mlp, alpha=alpha).cuda()
    # the mixed head by hand, from the two trained models as the construction left them (their predict biases zeroed, the reference's quirk);
    # pre's own LayerNorms are fresh (gamma 1, beta 0: not copied), so the MLP tower is evaluated with mlp's Linears and pre's LayerNorms
    users, cand, labels, counts = (torch.from_numpy(a).cuda() for a in valid)
    u, i = users[:, None].expand(-1, CANDS).reshape(-1), cand.reshape(-1)
    with torch.no_grad():
        gmf.eval(), mlp.eval(), pre.eval()
        x = torch.cat((mlp.embed_user_MLP(u), mlp.embed_item_MLP(i)), -1)
        for j, layer in enumerate(mlp.MLP_layers):
            x = pre.MLP_layers[j](x) if isinstance(layer, torch.nn.LayerNorm) else layer(x)
        feat = torch.cat((gmf.embed_user_GMF(u) * gmf.embed_item_GMF(i), x), -1)
        weight = torch.cat((alpha * gmf.predict_layer.weight, (1 - alpha) * mlp.predict_layer.weight), 1)
        by_hand = (feat @ weight.T).view(USERS, CANDS) + (alpha * gmf.predict_layer.bias + (1 - alpha) * mlp.predict_layer.bias)
        assert torch.equal(pre.predict_layer.weight, weight) and torch.allclose(pre((u, i)).view(USERS, CANDS), by_hand, rtol=1e-5, atol=1e-6)
    rm = RankingMetrics(users.device, USERS, (10, 20))
    rm.update(by_hand.contiguous(), labels, counts, 0)
    expect = rm.result()
    untouched = {k: v.detach().clone() for k, v in pre.state_dict().items() if k.startswith(("GMF_model.", "MLP_model."))}
    history = fit_ncf_model(pre, pairs, valid, max_epochs=1, **{**SETTINGS, "lr": 0.0})      # steps of size 0: the first validation is the built model's
    assert all(abs(history[0][k] - expect[k]) <= 1e-9 for k in ("n10", "n20", "r10", "r20")) and abs(history[0]["loss"] - expect["loss"]) <= 1e-5
    history = fit_ncf_model(pre, pairs, valid, max_epochs=2, **SETTINGS)      # and it trains: exactly as a NeuMF-end
    assert history[-1]["train_loss"] < history[0]["train_loss"]
    assert all(torch.equal(pre.state_dict()[k], v) for k, v in untouched.items())


def test_item_init_is_copied_in_and_refused_where_the_reference_refuses_it():
    pairs, valid = planted()
    init = torch.randn(ITEMS, 16, generator=torch.Generator().manual_seed(5))
    model = model_of("MLP")
    fit_ncf_model(model, pairs, valid, max_epochs=1, item_init=init.cuda(), freeze_items=True, **SETTINGS)
    assert torch.equal(model.embed_item_MLP.weight.detach().cpu(), init)      # copied in, then frozen: the same bits after an epoch
    model = model_of("MLP")
    fit_ncf_model(model, pairs, valid, max_epochs=1, item_init=init, **SETTINGS)
    assert not torch.equal(model.embed_item_MLP.weight.detach().cpu(), init)  # trained from there
    for kind in ("GMF", "NeuMF-pre"):
        extra = dict(GMF_model=model_of("GMF"), MLP_model=model_of("MLP")) if kind == "NeuMF-pre" else {}
        with pytest.raises(ValueError, match="item_init needs model kind"):
            fit_ncf_model(model_of(kind, **extra), pairs, valid, max_epochs=1, item_init=init, **SETTINGS)
    with pytest.raises(ValueError, match="item_init must be"):
        fit_ncf_model(model_of("MLP"), pairs, valid, max_epochs=1, item_init=init[:, :8], **SETTINGS)
    with pytest.raises(ValueError, match="early_criterion"):
        fit_ncf_model(model_of("MLP"), pairs, valid, max_epochs=1, early_criterion="auc", **SETTINGS)
