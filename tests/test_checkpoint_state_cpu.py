"""Host side of checkpoint / resume / fit (pmgt_amd/io.py, pmgt_amd/trainer.py), no GPU: the flat <-> per-parameter optimizer-state
mapping against the reference's grouping rule (pmgt/base_trainer.py:35-59, restated below over the reference's names), the file's
shape and its backward compatibility, the atomic write, the early-stopping / best-checkpoint bookkeeping on scripted metric sequences
and the epoch permutation.  Everything here is integer bookkeeping or a copy: comparisons are exact."""
import os

import numpy as np
import pytest
import torch

from oracle import pmgt_oracle as po
from pmgt_amd import io as pio
from pmgt_amd.trainer import BestCheckpoint, EarlyStopping, epoch_order, monitor_of

CFG = po.default_cfg(hidden_size=16, num_attention_heads=2, num_hidden_layers=2, intermediate_size=24, feat_hidden_sizes=[12, 8],
                     max_position_embeddings=10)
HP = {"lr": 1e-3, "weight_decay": 1e-2, "betas": (0.9, 0.999), "eps": 1e-8, "max_grad_norm": 5.0, "random_node_ratio": 0.02,
      "mask_node_ratio": 0.16, "schedule": ("linear", 2, 10)}


def make_entries(cfg=CFG, seed=0):
    """The reference's parameter names and shapes (oracle.param_shapes: named_parameters() order) laid out the way the engine lays
    its flat buffer out: in ANOTHER order than the reference's, every tensor on a 4-element boundary (so there are gaps)."""
    shapes = po.param_shapes(cfg)
    order = np.random.RandomState(seed).permutation(len(shapes))
    entries, cur = [], 0
    for i in order:
        name, shape = shapes[i]
        numel = int(np.prod(shape))
        entries.append(dict(name=name, offset=cur, numel=numel, shape=tuple(shape)))
        cur += -(-numel // 4) * 4 + 4 * (i % 2)
    return entries, cur


def covered(entries, n):
    mask = torch.zeros(n, dtype=torch.bool)
    for e in entries:
        mask[e["offset"]: e["offset"] + e["numel"]] = True
    return mask


def trainer_sd(entries, n, seed=1, opt_step=7, hp=HP):
    g = torch.Generator().manual_seed(seed)
    mask = covered(entries, n)
    rnd = lambda: torch.randn(n, generator=g) * mask
    eng = dict(n_params=n, dtype="fp32", config={"hidden_size": CFG["hidden_size"]}, params=rnd(), exp_avg=rnd(), exp_avg_sq=rnd().abs(),
               opt_step=opt_step, rng_state={"seed": 3, "step": 2 * opt_step}, options=["store_ln_input"])
    return {"engine": eng, "opt_steps": opt_step, "pipeline_step": 2 * opt_step, "hyper_parameters": dict(hp), "accumulate_grad_batches": 2}


def weights_of(entries, params, prefix="net."):
    return {prefix + e["name"]: params[e["offset"]: e["offset"] + e["numel"]].reshape(e["shape"]).clone() for e in entries}


def test_layout_round_trip_and_the_reference_groups():
    entries, n = make_entries()
    assert not bool(covered(entries, n).all())                                  # the layout has gaps, as the engine's has
    sd = trainer_sd(entries, n)["engine"]
    opt = pio.flat_to_optimizer_state(entries, sd["exp_avg"], sd["exp_avg_sq"], 7, 1e-3, 1e-2)
    # get_optimizer's rule over the names in named_parameters() order; the frozen feat_embeddings.* are not among them
    names = [nm for nm, _ in po.param_shapes(CFG)]
    no_decay = ["bias", "LayerNorm.weight"]
    g0 = [nm for nm in names if not any(nd in nm for nd in no_decay)]
    g1 = [nm for nm in names if any(nd in nm for nd in no_decay)]
    assert pio.optimizer_param_groups([e["name"] for e in entries]) == (g0, g1)
    assert not any("feat_embeddings" in nm for nm in g0 + g1)
    groups = opt["param_groups"]
    assert groups[0]["params"] == list(range(len(g0))) and groups[1]["params"] == list(range(len(g0), len(names)))
    assert groups[0]["weight_decay"] == 1e-2 and groups[1]["weight_decay"] == 0.0 and groups[0]["lr"] == groups[1]["lr"] == 1e-3
    by = {e["name"]: e for e in entries}
    for i, nm in enumerate(g0 + g1):
        st, e = opt["state"][i], by[nm]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and st["step"] == 7
        assert tuple(st["exp_avg"].shape) == e["shape"]
        assert torch.equal(st["exp_avg"].reshape(-1), sd["exp_avg"][e["offset"]: e["offset"] + e["numel"]])
    m, v, step = pio.optimizer_state_to_flat(entries, opt, n)
    assert step == 7 and torch.equal(m, sd["exp_avg"]) and torch.equal(v, sd["exp_avg_sq"])
    # a file of the reference lists the frozen tables behind the decayed parameters of group 0, without state
    shifted = {"state": {(i if i < len(g0) else i + 2): s for i, s in opt["state"].items()},
               "param_groups": [dict(groups[0], params=list(range(len(g0) + 2))),
                                dict(groups[1], params=list(range(len(g0) + 2, len(names) + 2)))]}
    m2, v2, step2 = pio.optimizer_state_to_flat(entries, shifted, n, n_frozen=2)
    assert step2 == 7 and torch.equal(m2, m) and torch.equal(v2, v)
    with pytest.raises(ValueError, match="parameter"):
        pio.optimizer_state_to_flat(entries[:-1], opt, n)


def test_file_shape_and_backward_compatibility(tmp_path):
    entries, n = make_entries()
    tsd = trainer_sd(entries, n)
    weights = weights_of(entries, tsd["engine"]["params"])
    weights["net.feat_embeddings.0.weight"] = torch.zeros(5, 12)
    ck = pio.training_checkpoint(weights, entries, tsd, epoch=2, callbacks={"EarlyStopping{'monitor': 'loss/val', 'mode': 'min'}": {"wait_count": 1}},
                                 fit={"epoch": 3, "batches_done": 0})
    path = tmp_path / "last.ckpt"
    pio.atomic_save(ck, path)
    got = torch.load(path, map_location="cpu", weights_only=True)                # the weights-only path is enough: plain data
    got2 = pio.read_checkpoint(str(path))
    for k in ("state_dict", "optimizer_states", "lr_schedulers", "global_step", "epoch", "callbacks", "pmgt_amd"):
        assert k in got and k in got2, k
    assert got["global_step"] == 7 and got["epoch"] == 2 and len(got["optimizer_states"]) == 1
    sched = got["lr_schedulers"]
    assert len(sched) == 1 and sched[0]["last_epoch"] == 7 and sched[0]["base_lrs"] == [1e-3, 1e-3]
    lam = (10 - 7) / (10 - 2)                                                   # linear, W = 2, T = 10 after 7 steps
    assert got["optimizer_states"][0]["param_groups"][0]["lr"] == pytest.approx(1e-3 * lam, rel=1e-12)
    assert got["optimizer_states"][0]["param_groups"][0]["initial_lr"] == 1e-3
    pv = got["pmgt_amd"]
    assert pv["format_version"] == pio.FORMAT_VERSION and pv["rng_state"] == {"seed": 3, "step": 14} and pv["opt_steps"] == 7
    assert pv["options"] == ["store_ln_input"] and pv["pipeline_step"] == 14 and pv["dtype"] == "fp32" and pv["fit"]["epoch"] == 3
    assert pio._callback(got["callbacks"], "EarlyStopping") == {"wait_count": 1}
    no_sched = pio.training_checkpoint(weights, entries, trainer_sd(entries, n, hp=dict(HP, schedule=None)))
    assert no_sched["lr_schedulers"] == [] and "initial_lr" not in no_sched["optimizer_states"][0]["param_groups"][0]

    class Sink:                                        # load_checkpoint reads the same file as before: the `net.` weights
        def load_state_dict(self, state, strict=True):
            self.state = state
            return "ok"
    sink = Sink()
    assert pio.load_checkpoint(sink, str(path)) == "ok"
    assert set(sink.state) == {k[4:] for k in weights}
    for k, v in weights.items():
        assert torch.equal(sink.state[k[4:]], v)
    # the pure part of the loader gives back what went in ...
    back = pio.training_state_from_checkpoint(got, entries, n, n_frozen=2)
    for k in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(back["engine"][k], tsd["engine"][k]), k
    assert back["engine"]["opt_step"] == 7 and back["engine"]["rng_state"] == {"seed": 3, "step": 14}
    assert back["hyper_parameters"] == HP and back["accumulate_grad_batches"] == 2 and back["opt_steps"] == 7 and back["pipeline_step"] == 14
    # ... and accepts a checkpoint without the private block (a Lightning file of the reference): weights, moments, step count
    foreign = {k: v for k, v in got.items() if k != "pmgt_amd"}
    back = pio.training_state_from_checkpoint(foreign, entries, n, n_frozen=2)
    for k in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(back["engine"][k], tsd["engine"][k]), k
    assert back["engine"]["opt_step"] == 7 and back["engine"]["rng_state"] is None and back["engine"]["options"] is None
    assert back["hyper_parameters"]["lr"] == 1e-3 and back["hyper_parameters"]["betas"] == (0.9, 0.999)
    assert "accumulate_grad_batches" not in back and "pipeline_step" not in back
    with pytest.raises(ValueError, match="newer"):
        pio.training_state_from_checkpoint(dict(got, pmgt_amd=dict(pv, format_version=pio.FORMAT_VERSION + 1)), entries, n)


def test_a_failed_write_leaves_the_previous_file_intact(tmp_path, monkeypatch):
    path = tmp_path / "last.ckpt"
    pio.atomic_save({"generation": 1, "w": torch.arange(4.0)}, path)
    before = path.read_bytes()

    def killed(src, dst):
        assert os.path.exists(src) and os.path.dirname(src) == os.path.dirname(dst)       # written next to the target, not yet renamed
        raise KeyboardInterrupt("killed between write and rename")
    monkeypatch.setattr(os, "replace", killed)
    with pytest.raises(KeyboardInterrupt):
        pio.atomic_save({"generation": 2, "w": torch.arange(8.0)}, path)
    monkeypatch.undo()
    assert path.read_bytes() == before
    assert torch.load(path, weights_only=True)["generation"] == 1
    assert os.listdir(tmp_path) == ["last.ckpt"]                                          # and no temporary file stays behind
    real_save = torch.save

    def half_written(obj, f, *a, **k):
        with open(f, "wb") as fh:
            fh.write(b"half a file")
        raise OSError("disk full")
    monkeypatch.setattr(torch, "save", half_written)
    with pytest.raises(OSError):
        pio.atomic_save({"generation": 3}, path)
    monkeypatch.setattr(torch, "save", real_save)
    assert path.read_bytes() == before and os.listdir(tmp_path) == ["last.ckpt"]


@pytest.mark.parametrize("criterion,sign", [("loss", 1.0), ("auc", -1.0)])
def test_early_stopping_and_best_checkpoint_bookkeeping(criterion, sign):
    monitor, mode = monitor_of(criterion)
    assert (monitor, mode) == (("loss/val", "min") if criterion == "loss" else ("val/auc", "max"))
    # written for "min"; mirrored for "max".  improvement, improvement, tie, worse, improvement, worse, tie with the best, worse
    script = [0.9, 0.8, 0.8, 0.85, 0.7, 0.75, 0.7, 0.9]
    values = [v if sign > 0 else 1.0 - v for v in script]
    want_wait = [0, 0, 1, 2, 0, 1, 2, 3]
    es, bc = EarlyStopping(monitor, 3, mode), BestCheckpoint("/ck", monitor, mode)
    stops, waits, writes, removes = [], [], [], []
    for ep, v in enumerate(values):
        w, r = bc.update(ep, v)
        stops.append(es.update(v, ep))
        waits.append(es.wait_count)
        writes.append(w)
        removes.append(r)
    assert waits == want_wait                                                  # a tie counts as no improvement
    assert stops == [False] * 7 + [True] and es.stopped_epoch == 7
    short = criterion
    name = lambda ep: f"/ck/epoch={ep:02d}-{short}={values[ep]:.4f}.ckpt"
    assert writes == [name(0), name(1), None, None, name(4), None, None, None]
    assert removes == [None, name(0), None, None, name(1), None, None, None]   # one best file at a time
    assert bc.best_model_path == name(4) and bc.best_model_score == values[4] and es.best_score == values[4]
    assert name(4) == ("/ck/epoch=04-loss=0.7000.ckpt" if criterion == "loss" else "/ck/epoch=04-auc=0.3000.ckpt")
    # patience 1: the first non-improving validation stops
    es1 = EarlyStopping(monitor, 1, mode)
    assert [es1.update(v) for v in values[:3]] == [False, False, True]
    # the state survives a checkpoint: a restored pair continues the count
    es2, bc2 = EarlyStopping(monitor, 3, mode), BestCheckpoint("/ck", monitor, mode)
    es3, bc3 = EarlyStopping(monitor, 3, mode), BestCheckpoint("/ck", monitor, mode)
    for ep, v in enumerate(values[:6]):
        bc2.update(ep, v)
        es2.update(v, ep)
    es3.load_state_dict(es2.state_dict())
    bc3.load_state_dict(bc2.state_dict())
    assert (es3.wait_count, es3.best_score, bc3.best_model_path, bc3.best_model_score) == (1, values[4], name(4), values[4])
    assert [es3.update(v, 6 + i) for i, v in enumerate(values[6:])] == [False, True]
    assert es.state_key.startswith("EarlyStopping") and bc.state_key.startswith("ModelCheckpoint")


def test_epoch_permutation_is_a_pure_function_and_covers_the_shard_once():
    n = 103
    for world in (1, 2, 4):
        for epoch in (0, 1, 5):
            parts = [epoch_order(n, 11, epoch, r, world) for r in range(world)]
            again = [epoch_order(n, 11, epoch, r, world) for r in range(world)]
            assert all(np.array_equal(a, b) for a, b in zip(parts, again))
            per_rank = -(-n // world)
            assert all(len(p) == per_rank for p in parts)                       # every rank runs the same number of steps
            allidx = np.concatenate(parts)
            counts = np.bincount(allidx, minlength=n)
            assert counts.min() == 1 and counts.sum() == per_rank * world       # every id once; the wrap-around pad repeats a few
            assert (counts > 1).sum() == per_rank * world - n
            if world == 1:
                assert sorted(parts[0].tolist()) == list(range(n))
    assert not np.array_equal(epoch_order(n, 11, 0), epoch_order(n, 11, 1))    # epochs differ
    assert not np.array_equal(epoch_order(n, 11, 0), epoch_order(n, 12, 0))    # seeds differ
    # ranks interleave ONE permutation: rank r holds elements r, r + W, ... of it
    whole = epoch_order(n - 1, 3, 2)
    assert np.array_equal(epoch_order(n - 1, 3, 2, 1, 2), whole[1::2])
