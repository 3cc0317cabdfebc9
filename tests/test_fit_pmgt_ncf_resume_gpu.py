"""fit_pmgt_ncf with last.ckpt, resume and graph replay, in the world of tests/test_fit_pmgt_ncf_gpu.py (48 items, 16 users, hidden 64,
2 layers, S 16, batch 32, 4 epochs) built with hidden_dropout_prob = 0.1, so that engine.rng_state matters to every step.

  * A run preempted after two epochs and resumed in a NEW model is the uninterrupted run BIT FOR BIT: the history, every bert.* and head
    tensor of the final model, the best file and last.ckpt -- with the defaults, and with SGD under a linear schedule with warm-up, the guard
    and a step log.
  * graph=True gives graph=False's history and final tensors bit for bit, also when a short last batch runs eagerly between replays.
  * A resume under another batch_size, num_ng, seed, early_criterion or patience (with a schedule, max_epochs) is refused with both values
    named; a foreign file and save_last without ckpt_dir are refused; a stopped file returns its history and takes no step."""
import glob
import os

import numpy as np
import pytest
import torch

from pmgt_amd import finetune
from pmgt_amd.finetune import LAST_FORMAT, fit_pmgt_ncf
from pmgt_amd.pair_train import pair_schedule_steps
from tests.test_fit_pmgt_ncf_gpu import BATCH, EPOCHS, LR, N_ITEMS, N_USERS, NUM_NG, S, tensors_of

pytestmark = pytest.mark.gpu

OPTIONS = dict(optim="sgd", scheduler_type="linear", scheduler_warmup=0.1, nonfinite="skip", step_log=8, lr=0.02)


class Preempted(Exception):
    pass


def stop_after_epoch_1(row):
    if row["epoch"] == 1:
        raise Preempted


def build():
    """build() of tests/test_fit_pmgt_ncf_gpu.py with the encoder's dropout on"""
    from pmgt_amd.configuration_pmgt import PMGTConfig
    from pmgt_amd.datasets import MCNSampler, ranking_candidates
    from pmgt_amd.graph import synthetic_graph
    from pmgt_amd.models import synthetic_features
    from pmgt_amd.pmgt_ncf import PMGT_NCF
    torch.manual_seed(0)
    cfg = PMGTConfig(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=64, feat_hidden_sizes=(32, 16),
                     hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.0)
    model = PMGT_NCF(user_num=N_USERS, item_num=N_ITEMS, factor_num=16, num_layers=3, model="NeuMF-end", config=cfg, dtype="fp32")
    feats = synthetic_features(N_ITEMS, (32, 16), seed=1)
    for f in feats:
        f[2 + N_ITEMS // 2:, : f.shape[1] // 2] += 1.5
    model.set_features(feats)
    sampler = MCNSampler(synthetic_graph(N_ITEMS, 200, seed=2), max_ctx_neigh=S - 1)
    rng = np.random.default_rng(3)
    train, valid = [], []
    for u in range(N_USERS):
        mine = (u % 2) * (N_ITEMS // 2) + rng.choice(N_ITEMS // 2, size=10, replace=False)
        train += [(u, int(i)) for i in mine[:8]]
        valid += [(u, int(i)) for i in mine[8:]]
    return model, sampler, np.asarray(train), ranking_candidates(valid, N_USERS, N_ITEMS, 20, seed=4)


def run(ckpt_dir, **kw):
    """one fit on a NEW model -> (history, the final model's tensors)"""
    model, sampler, train, valid = build()
    args = dict(batch_size=BATCH, max_epochs=EPOCHS, num_ng=NUM_NG, seed=0, lr=LR, patience=10, ckpt_dir=ckpt_dir,
                save_last=ckpt_dir is not None)
    args.update(kw)
    history = fit_pmgt_ncf(model, sampler, train, valid, **args)
    return history, tensors_of(model)


def same(a, b, what):
    """equal structure, equal values, tensors bit for bit"""
    assert type(a) is type(b) or (isinstance(a, (list, tuple)) and isinstance(b, (list, tuple))), (what, type(a), type(b))
    if isinstance(a, dict):
        assert set(a) == set(b), (what, set(a) ^ set(b))
        for k in a:
            same(a[k], b[k], f"{what}[{k!r}]")
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{what}[{i}]")
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu().reshape(-1).view(torch.uint8), b.cpu().reshape(-1).view(torch.uint8)), what
    else:
        assert a == b, (what, a, b)


def strip_dir(ck, ckpt_dir):
    """a last.ckpt without the folder it lies in"""
    ck = dict(ck, best_checkpoint=dict(ck["best_checkpoint"]))
    for k in ("best_model_path", "dirpath", "last_model_path"):
        ck["best_checkpoint"][k] = os.path.relpath(ck["best_checkpoint"][k], ckpt_dir) if ck["best_checkpoint"][k] else ""
    return ck


@pytest.mark.parametrize("options", [{}, OPTIONS], ids=["defaults", "sgd-linear-guard"])
def test_a_resumed_run_is_the_uninterrupted_run_bit_for_bit(options, tmp_path):
    dir_a, dir_b = str(tmp_path / "a"), str(tmp_path / "b")
    hist_a, model_a = run(dir_a, **options)
    assert len(hist_a) == EPOCHS and all(np.isfinite(h["train_loss"]) for h in hist_a) and hist_a[-1]["train_loss"] != hist_a[0]["train_loss"]
    seen = []
    with pytest.raises(Preempted):
        run(dir_b, log=lambda row: (seen.append(row), stop_after_epoch_1(row)), **options)
    assert [r["epoch"] for r in seen] == [0, 1]
    part = torch.load(os.path.join(dir_b, "last.ckpt"), weights_only=True)      # plain data; written BEFORE log raised
    assert part["format"] == LAST_FORMAT and part["epoch"] == 1 and len(part["history"]) == 2 and not part["stopped"]
    total, warmup = pair_schedule_steps(N_USERS * 8, NUM_NG, BATCH, EPOCHS, options.get("scheduler_warmup"))
    assert int(part["trainer"]["step"][0]) == total // EPOCHS * 2
    if options:
        assert part["trainer"]["optim"] == "sgd" and part["trainer"]["schedule"] == ("linear", warmup, total) and warmup == int(0.1 * total)
        assert part["run"]["max_epochs"] == EPOCHS and part["trainer"]["step_counters"].tolist() == [total // EPOCHS * 2, 0, 0, 0]
        assert "exp_avg" not in part["trainer"] and "exp_avg" not in part["trainer"]["encoder"]
    else:
        assert set(part["trainer"]) == {"params", "step", "layout", "exp_avg", "exp_avg_sq", "encoder"} and "max_epochs" not in part["run"]
    resumed = []
    hist_b, model_b = run(dir_b, log=resumed.append, resume_from="last", **options)      # a NEW model: everything comes from the file
    assert [r["epoch"] for r in resumed] == [2, 3]
    same(hist_a, hist_b, "history")
    same(model_a, model_b, "the final model")
    assert any(k.startswith("bert.encoder") for k in model_a) and "gmf_item_embeddings.weight" in model_a
    last_a, last_b = (torch.load(os.path.join(d, "last.ckpt"), weights_only=True) for d in (dir_a, dir_b))
    assert last_a["epoch"] == EPOCHS - 1 and int(last_a["trainer"]["step"][0]) == total
    same(strip_dir(last_a, dir_a), strip_dir(last_b, dir_b), "last.ckpt")      # the state, engine.rng_state in it, the callbacks, the best ranges
    files_a, files_b = (sorted(os.path.basename(f) for f in glob.glob(os.path.join(d, "*"))) for d in (dir_a, dir_b))
    assert files_a == files_b and len(files_a) == 2 and "last.ckpt" in files_a
    best = next(f for f in files_a if f != "last.ckpt")
    same(torch.load(os.path.join(dir_a, best), weights_only=False), torch.load(os.path.join(dir_b, best), weights_only=False), "the best file")


@pytest.mark.parametrize("options", [{}, OPTIONS], ids=["defaults", "sgd-linear-guard"])
@pytest.mark.parametrize("batch,epochs", [(BATCH, EPOCHS), (40, 2)], ids=["batch32", "batch40-short-last"])
def test_graph_replay_gives_the_eager_history_and_tensors(batch, epochs, options):
    n_rows = N_USERS * 8 * (1 + NUM_NG)
    assert (n_rows % batch != 0) == (batch == 40)            # at 40 the last batch of an epoch is short and runs eagerly
    hist_e, model_e = run(None, batch_size=batch, max_epochs=epochs, **options)
    hist_g, model_g = run(None, batch_size=batch, max_epochs=epochs, graph=True, **options)
    same(hist_e, hist_g, "history")
    same(model_e, model_g, "the final model")
    assert len(hist_e) == epochs and hist_e[-1]["train_loss"] != hist_e[0]["train_loss"]


def test_refusals_and_a_stopped_file(tmp_path, monkeypatch):
    ckpt_dir = str(tmp_path / "run")
    opts = dict(OPTIONS, max_epochs=2)
    with pytest.raises(Preempted):
        run(ckpt_dir, log=lambda row: stop_after_epoch_1(dict(row, epoch=row["epoch"] + 1)), **opts)      # stopped after epoch 0
    for kw, key in ((dict(batch_size=16), "batch_size"), (dict(num_ng=1), "num_ng"), (dict(seed=4), "seed"), (dict(early_criterion="r20"), "early_criterion"),
                    (dict(patience=2), "patience"), (dict(max_epochs=3), "max_epochs")):
        with pytest.raises(ValueError, match=rf"written with {key} = .*this call has"):
            run(ckpt_dir, resume_from="last", **{**opts, **kw})
    with pytest.raises(ValueError, match="schedule"):        # another schedule, another optimizer: the trainer's refusals
        run(ckpt_dir, resume_from="last", **dict(opts, scheduler_type="cosine"))
    with pytest.raises(ValueError, match="optim"):
        run(ckpt_dir, resume_from="last", **dict(opts, optim="adamw"))
    best = next(f for f in glob.glob(os.path.join(ckpt_dir, "*.ckpt")) if not f.endswith("last.ckpt"))
    with pytest.raises(ValueError, match="not written by fit_pmgt_ncf"):
        run(ckpt_dir, resume_from=best, **opts)
    with pytest.raises(ValueError, match="ckpt_dir"):
        run(None, save_last=True, **opts)
    # a run that early stopping ended: the file says so, and a resume returns its history without a step
    real = finetune.ranking_validator

    def worsening(*args, **kw):
        validate = real(*args, **kw)
        return lambda epoch: dict(validate(epoch), n20=1.0 / (1 + epoch))
    monkeypatch.setattr(finetune, "ranking_validator", worsening)
    done = str(tmp_path / "done")
    hist, model_a = run(done, patience=1)
    assert [h["best"] for h in hist] == [True, False] and torch.load(os.path.join(done, "last.ckpt"), weights_only=True)["stopped"]

    def no_step(*args, **kw):
        raise AssertionError("a stopped run takes no step")
    monkeypatch.setattr(finetune.PmgtNcfTrainer, "step", no_step)
    again, model_b = run(done, patience=1, resume_from="last", save_last=False)
    same(hist, again, "history")
    same(model_a, model_b, "the best epoch's model, restored")
