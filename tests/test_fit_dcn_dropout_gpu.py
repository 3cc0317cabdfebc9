"""fit_dcn(dropout_seed=...) in the world and with the settings of tests/test_fit_dcn_gpu.py, the model built the way the reference's
scripts/run_dcn.sh builds it: emb_dropout = 0.2, dropout = 0.  The training steps are training-mode steps (the emb mask drawn inside the
fused launches from the device {seed, step} pair), validation stays eval-mode.

THE BOUND on the best validation AUC comes from the torch yardstick of the same procedure WITH TORCH'S OWN DROPOUT (torch_fit_dropout
below: test_fit_dcn_gpu.torch_fit with the model in train() during the steps and in eval() for the validation; nn.Dropout draws from the
torch generator the seed sets) over the torch seeds 0 .. 5, on the CPU: the worst seed minus the spread (max - min),
    seed       0       1       2       3       4       5
    best       0.8534  0.8678  0.8650  0.8458  0.8295  0.8466
    bound = min - (max - min) = 0.8295 - 0.0383 = 0.7911
(python -m tests.test_fit_dcn_dropout_gpu prints them again; no GPU is needed for that.)"""
import numpy as np
import pytest
import torch

from pmgt_amd.dcn import DCN
from pmgt_amd.dcn_train import validation_seed
from tests.test_fit_dcn_gpu import EPOCHS, ITEMS, SEEDS, SETTINGS, SHAPE, USERS, pair_lists

EMB_DROPOUT, DROPOUT, DROPOUT_SEED = 0.2, 0.0, 20240607
SEED_BEST = (0.8534, 0.8678, 0.8650, 0.8458, 0.8295, 0.8466)      # torch seeds 0 .. 5
AUC_BOUND = min(SEED_BEST) - (max(SEED_BEST) - min(SEED_BEST))


def make_model(torch_seed):
    torch.manual_seed(torch_seed)
    return DCN(USERS, ITEMS, *SHAPE[:3], emb_dropout=EMB_DROPOUT, dropout=DROPOUT, use_layer_norm=SHAPE[3], layer_norm_eps=1e-12)


def torch_fit_dropout(torch_seed, epochs=EPOCHS):
    """fit_dcn's loop on the CPU in fp32 torch with nn.Dropout -> the validation AUC after every epoch."""
    from pmgt_amd.evaluation import roc_auc_score
    from pmgt_amd.fit_loop import epoch_order
    from pmgt_amd.ncf_train import ng_sample
    train, valid = pair_lists()
    model = make_model(torch_seed)
    named = list(model.named_parameters())
    opt = torch.optim.AdamW([{"params": [p for k, p in named if "bias" not in k], "weight_decay": SETTINGS["weight_decay"]},
                             {"params": [p for k, p in named if "bias" in k], "weight_decay": 0.0}], lr=SETTINGS["lr"])
    vu, vi, vl = ng_sample(valid, USERS, ITEMS, SETTINGS["max_sample_items"], validation_seed(SETTINGS["seed"]))
    aucs = []
    for epoch in range(epochs):
        users, items, labels = ng_sample(train, USERS, ITEMS, SETTINGS["num_ng"], SETTINGS["seed"] + epoch)
        order = epoch_order(len(users), SETTINGS["seed"], epoch)
        users, items, labels = (torch.from_numpy(a[order]) for a in (users, items, labels))
        model.train()
        for lo in range(0, len(order), SETTINGS["batch_size"]):
            hi = lo + SETTINGS["batch_size"]
            opt.zero_grad(set_to_none=True)
            torch.nn.functional.binary_cross_entropy_with_logits(model((users[lo:hi], items[lo:hi])), labels[lo:hi]).backward()
            torch.nn.utils.clip_grad_norm_([p for _, p in named if p.grad is not None], SETTINGS["max_grad_norm"])
            opt.step()
        model.eval()
        with torch.no_grad():
            scores = torch.sigmoid(model((torch.from_numpy(vu), torch.from_numpy(vi)))).numpy()
        aucs.append(roc_auc_score(vl, scores))
    return aucs


@pytest.mark.gpu
def test_fit_with_the_script_s_dropout_learns_and_is_a_pure_function_of_the_seed():
    from pmgt_amd import evaluate_ctr, fit_dcn
    from pmgt_amd.ncf_train import ng_sample
    train, valid = pair_lists()
    model = make_model(0).cuda().train()                     # (the fit takes training-mode steps and validates in eval mode whatever this says)
    history = fit_dcn(model, train, valid, max_epochs=EPOCHS, early_criterion="auc", patience=EPOCHS, dropout_seed=DROPOUT_SEED, **SETTINGS)
    assert model.training and len(history) == EPOCHS
    assert all(np.isfinite(h[k]) for h in history for k in ("train_loss", "auc", "loss")) and all(0 <= h["auc"] <= 1 for h in history)
    best = max((h for h in history if h["best"]), key=lambda h: h["epoch"])
    print("auc " + " ".join(f"{h['auc']:.4f}" for h in history) + f"; train loss {history[0]['train_loss']:.4f} -> {history[-1]['train_loss']:.4f}")
    assert best["auc"] == max(h["auc"] for h in history) and best["auc"] >= AUC_BOUND and best["auc"] > history[0]["auc"] and best["epoch"] > 0
    assert history[-1]["train_loss"] < history[0]["train_loss"]
    # the model holds the best parameters, and the evaluation of a model trained with its dropout is eval-mode: no mask, the same number twice
    vu, vi, vl = ng_sample(valid, USERS, ITEMS, SETTINGS["max_sample_items"], validation_seed(SETTINGS["seed"]))
    ev = evaluate_ctr(model, vu, vi, vl, batch_size=100)
    assert ev == evaluate_ctr(model, vu, vi, vl, batch_size=100) and ev["auc"] == best["auc"] and ev["loss"] == best["loss"]
    # one seed, one history; another seed, another
    again = fit_dcn(make_model(0).cuda(), train, valid, max_epochs=EPOCHS, early_criterion="auc", patience=EPOCHS, dropout_seed=DROPOUT_SEED,
                    **SETTINGS)
    assert again == history
    other = fit_dcn(make_model(0).cuda(), train, valid, max_epochs=2, early_criterion="auc", patience=EPOCHS, dropout_seed=DROPOUT_SEED + 1,
                    **SETTINGS)
    assert other[0]["train_loss"] != history[0]["train_loss"]
    with pytest.raises(ValueError, match="dropout is not covered"):
        fit_dcn(make_model(0).cuda(), train, valid, max_epochs=1, **SETTINGS)
    with pytest.raises(ValueError, match="dropout is not covered"):      # a model no seeded trainer holds is still refused by the evaluation
        evaluate_ctr(make_model(0).cuda(), vu, vi, vl)


if __name__ == "__main__":
    runs = [torch_fit_dropout(s) for s in SEEDS]
    best = [max(r) for r in runs]
    print("best  " + "  ".join(f"{b:.4f}" for b in best))
    print(f"bound = {min(best):.4f} - {max(best) - min(best):.4f} = {min(best) - (max(best) - min(best)):.4f}")
    for r in runs:
        print(" ".join(f"{a:.3f}" for a in r))
