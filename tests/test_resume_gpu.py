"""Checkpoint / resume of the full training state and the fit loop, on the device (pmgt_amd/engine.py training_state, pmgt_amd/trainer.py
state_dict / load_state_dict / run_live(first_step) / fit, pmgt_amd/io.py save_training_checkpoint / load_training_checkpoint).

Bounds.  A resumed run against the uninterrupted one: bit for bit (torch.equal on parameters, both moments, opt_step, rng_state; == on
every later loss and pre-clip gradient norm) -- the engine's reductions are fixed-order and nothing but the saved state enters a step.
Dropout is ON (0.1 / 0.1) wherever the fixture allows it, so a wrong rng_state shows.  The comparison with the reference's curve uses the
bounds of tests/test_engine_gpu.py::test_clip_adamw_curve_matches_reference for the same fixtures (loss rtol 2e-4, gradient norm rtol
1e-3, final parameters 2e-3 / 2e-5)."""
import copy
import os
import re
import socket

import numpy as np
import pytest
import torch

from oracle import pmgt_oracle as po
from tests import golden_util as gu
from tests.test_engine_gpu import dev_batch, inject_for, make_engine

pytestmark = pytest.mark.gpu

DROP = dict(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
KW = dict(lr=1e-3, weight_decay=1e-2, max_grad_norm=5.0, scheduler_type="linear", num_warmup_steps=2, num_training_steps=12)


@pytest.fixture(autouse=True)
def _no_graph_left_behind():
    """Captured steps are destroyed here, with the GPU idle (see tests/test_lr_schedule_gpu.py)."""
    yield
    import gc
    torch.cuda.synchronize()
    gc.collect()


def fresh_engine(case, dtype, seed=0, **cfg_over):
    """An engine built from the configuration alone: feature tables (a dataset input), NO parameters."""
    from pmgt_amd.configuration_pmgt import PMGTConfig
    from pmgt_amd.engine import Engine
    cfg = dict(case["cfg"])
    cfg.update(cfg_over)
    eng = Engine(PMGTConfig(**cfg), dtype=dtype, seed=seed)
    eng.set_tables(*[t.numpy() for t in case["tables"]])
    return eng


def state_of(eng):
    torch.cuda.synchronize()
    return dict(params=eng.params.clone(), exp_avg=eng.exp_avg.clone(), exp_avg_sq=eng.exp_avg_sq.clone(), opt_step=eng.opt_step.clone(),
                rng_state=eng.rng_state.clone())


def assert_same_state(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]), k


def run_steps(tr, batch, n):
    """n micro-batches -> [(loss, pre-clip gradient norm of the optimizer step it completed, or None)]"""
    out = []
    for _ in range(n):
        loss = tr.train_step(batch).item()
        out.append((loss, tr.engine.grad_norm().item() if tr._micro == 0 else None))
    return out


class WeightsOnly:
    """What load_checkpoint hands the weights to, over a bare engine."""

    def __init__(self, eng):
        self.eng = eng

    def load_state_dict(self, state, strict=True):
        self.eng.load_params(state)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_eager_resume_from_disk_into_a_fresh_engine_is_bit_identical(dtype, tmp_path):
    """12 micro-batches (accumulation 2: 6 optimizer steps, linear schedule with warm-up, clip) uninterrupted, against 6 -> file -> a fresh
    Engine and Trainer built from the configuration and the file alone (another seed: the file's must win) -> 6.  Then the negative control:
    the same file through load_checkpoint (weights only) must NOT continue the curve -- the test can see a lost moment / counter."""
    from pmgt_amd import io as pio
    from pmgt_amd.trainer import Trainer
    case = gu.model_case("m3")
    batch = dev_batch(case["batch"])
    N, K = 12, 6
    eng_a = make_engine(case, dtype=dtype, **DROP)
    tr_a = Trainer(eng_a, accumulate_grad_batches=2, **KW)
    curve_a = run_steps(tr_a, batch, N)
    final_a = state_of(eng_a)
    assert int(final_a["opt_step"]) == N // 2 and final_a["rng_state"].tolist()[1] > 0

    eng_b = make_engine(case, dtype=dtype, **DROP)
    tr_b = Trainer(eng_b, accumulate_grad_batches=2, **KW)
    assert run_steps(tr_b, batch, K) == curve_a[:K]
    path = tmp_path / "last.ckpt"
    pio.save_training_checkpoint(eng_b, tr_b, path)
    del eng_b, tr_b
    eng_c = fresh_engine(case, dtype, seed=99, **DROP)
    tr_c = Trainer(eng_c, accumulate_grad_batches=2, **KW)
    ck = pio.load_training_checkpoint(eng_c, tr_c, str(path))
    assert ck["global_step"] == K // 2 and tr_c._opt_steps == K // 2
    curve_c = run_steps(tr_c, batch, N - K)
    assert curve_c == curve_a[K:]                      # every later loss and gradient norm, exactly
    assert_same_state(final_a, state_of(eng_c))

    eng_d = fresh_engine(case, dtype, seed=0, **DROP)
    pio.load_checkpoint(WeightsOnly(eng_d), str(path))
    assert torch.equal(eng_d.params, torch.as_tensor(pio.training_state_from_checkpoint(ck, eng_d.entries, eng_d.n_params)["engine"]["params"]).cuda())
    tr_d = Trainer(eng_d, accumulate_grad_batches=2, **KW)
    curve_d = run_steps(tr_d, batch, N - K)
    torch.cuda.synchronize()
    assert curve_d[0][0] != curve_a[K][0] or not torch.equal(eng_d.params, final_a["params"])
    assert not torch.equal(eng_d.params, final_a["params"])


def test_saving_inside_an_accumulation_window_raises(tmp_path):
    from pmgt_amd import io as pio
    from pmgt_amd.trainer import Trainer
    case = gu.model_case("m3")
    batch = dev_batch(case["batch"])
    eng = make_engine(case, dtype="bf16", **DROP)
    tr = Trainer(eng, accumulate_grad_batches=2, **KW)
    tr.train_step(batch)
    with pytest.raises(RuntimeError, match="optimizer-step boundary"):
        tr.state_dict()
    with pytest.raises(RuntimeError, match="optimizer-step boundary"):
        pio.save_training_checkpoint(eng, tr, tmp_path / "x.ckpt")
    assert not os.path.exists(tmp_path / "x.ckpt")
    tr.train_step(batch)
    tr.state_dict()


def test_mismatches_are_named_or_refused():
    from pmgt_amd.trainer import Trainer
    case = gu.model_case("m3")
    batch = dev_batch(case["batch"])
    eng = make_engine(case, dtype="fp32", **DROP)
    tr = Trainer(eng, **KW)
    run_steps(tr, batch, 2)
    sd = tr.state_dict()
    want = state_of(eng)
    # a hyper-parameter: both values in the message; strict=False takes the tensors and keeps the trainer's value
    for over, name, a, b in ((dict(lr=2e-3), "lr", "0.001", "0.002"), (dict(max_grad_norm=1.0), "max_grad_norm", "5.0", "1.0"),
                             (dict(weight_decay=0.0), "weight_decay", "0.01", "0.0"), (dict(num_training_steps=20), "schedule", "12", "20"),
                             (dict(betas=(0.8, 0.999)), "betas", "0.9", "0.8"), (dict(eps=1e-6), "eps", "1e-08", "1e-06")):
        eng2 = fresh_engine(case, "fp32", **DROP)
        tr2 = Trainer(eng2, **dict(KW, **over))
        with pytest.raises(ValueError) as ei:
            tr2.load_state_dict(sd)
        assert f"{name}: checkpoint " in str(ei.value) and a in str(ei.value) and b in str(ei.value), str(ei.value)
        assert float(eng2.params.abs().max()) == 0.0                 # refused before anything was written
    tr2.load_state_dict(sd, strict=False)
    assert_same_state(want, state_of(eng2))
    assert tr2.eps == 1e-6 and tr2._opt_steps == 2
    eng3 = fresh_engine(case, "fp32", **DROP)
    tr3 = Trainer(eng3, accumulate_grad_batches=2, **KW)
    with pytest.raises(ValueError, match="accumulate_grad_batches: checkpoint 1, trainer 2"):
        tr3.load_state_dict(sd)
    # shapes: another parameter count, another engine dtype, another configuration with the same count -- refused with strict=False too
    eng4 = fresh_engine(case, "fp32", intermediate_size=128, **DROP)
    with pytest.raises(ValueError, match=f"{eng.n_params} parameters.*{eng4.n_params}"):
        Trainer(eng4, **KW).load_state_dict(sd, strict=False)
    eng5 = fresh_engine(case, "bf16", **DROP)
    with pytest.raises(ValueError, match="'fp32'.*'bf16'"):
        Trainer(eng5, **KW).load_state_dict(sd, strict=False)
    eng6 = fresh_engine(case, "fp32", hidden_dropout_prob=0.2, attention_probs_dropout_prob=0.1)
    with pytest.raises(ValueError, match="hidden_dropout_prob"):
        Trainer(eng6, **KW).load_state_dict(sd, strict=False)
    for e in (eng4, eng5, eng6):
        assert float(e.params.abs().max()) == 0.0 and e.exp_avg is None


def live_inputs(case, n_ids):
    from pmgt_amd.datasets import MCNSampler
    from pmgt_amd.graph import synthetic_graph
    n = case["n_nodes"]
    S = case["batch"][0]["node_ids"].shape[1]
    return MCNSampler(synthetic_graph(n, 5 * n, seed=3), S - 1), np.arange(2, 2 + n_ids)


def test_loading_in_place_keeps_captured_steps_valid(monkeypatch):
    """3 captured steps alive (one per pipeline slot); a state saved after step 3 is loaded after step 6: the SAME captures replay steps 4 - 6
    again and land on the same bits, which are also those of an eager continuation of that state in a fresh engine.  A state saved under
    another lr drops the captures."""
    from pmgt_amd.trainer import Trainer
    case = gu.model_case("m3")
    smp, ids = live_inputs(case, 128)
    live = dict(batch_size=32, threads=2, depth=3)
    eng = make_engine(case, dtype="bf16", **DROP)
    tr = Trainer(eng, **KW)
    captures = []
    orig = Trainer.capture_step
    monkeypatch.setattr(Trainer, "capture_step", lambda self, *a, **k: (captures.append(1), orig(self, *a, **k))[1])
    tr.run_live(smp, ids, steps=3, graphs=True, **live)
    assert len(captures) == 3 and len(tr._live_replays) == 3 and tr.pipeline_step == 3
    sd = tr.state_dict()
    saved = state_of(eng)
    buffers = [t.data_ptr() for t in (eng.params, eng.exp_avg, eng.exp_avg_sq, eng.opt_step, eng.rng_state)]
    tr.run_live(smp, ids, steps=3, graphs=True, first_step=3, **live)
    first = state_of(eng)
    loss_first = tr.last_loss.item()
    assert int(first["opt_step"]) == 6 and len(captures) == 3 and not torch.equal(first["params"], saved["params"])
    tr.load_state_dict(sd)
    assert [t.data_ptr() for t in (eng.params, eng.exp_avg, eng.exp_avg_sq, eng.opt_step, eng.rng_state)] == buffers      # written, not rebound
    assert_same_state(saved, state_of(eng))
    assert len(tr._live_replays) == 3 and tr.pipeline_step == 3 and tr._opt_steps == sd["opt_steps"]
    tr.run_live(smp, ids, steps=3, graphs=True, first_step=tr.pipeline_step, **live)
    assert len(captures) == 3                           # equal hyper-parameters: no re-capture
    assert_same_state(first, state_of(eng))
    assert tr.last_loss.item() == loss_first
    # the eager continuation of the same state, in another engine
    eng_e = fresh_engine(case, "bf16", seed=5, **DROP)
    tr_e = Trainer(eng_e, **KW)
    tr_e.load_state_dict(sd)
    tr_e.run_live(smp, ids, steps=3, graphs=False, first_step=tr_e.pipeline_step, **live)
    assert len(captures) == 3
    assert_same_state(first, state_of(eng_e))
    assert tr_e.last_loss.item() == loss_first
    # another lr: frozen into the captured launches, so they go
    other = copy.deepcopy(sd)
    other["hyper_parameters"]["lr"] = 5e-4
    with pytest.raises(ValueError, match="lr: checkpoint 0.0005, trainer 0.001"):
        tr.load_state_dict(other)
    assert len(tr._live_replays) == 0
    tr.run_live(smp, ids, steps=3, graphs=True, first_step=3, **live)
    assert len(captures) == 6 and len(tr._live_replays) == 3
    tr.load_state_dict(other, strict=False)
    assert len(tr._live_replays) == 0 and tr.lr == 1e-3
    assert_same_state(saved, state_of(eng))
    tr.drop_captured_steps()


def test_run_live_continues_with_first_step_and_restarts_without():
    """n = (s + 1) * batch_size ids, so that step s of one call and step 0 of the next take the same slice of node_ids."""
    from pmgt_amd.trainer import Trainer
    case = gu.model_case("m3")
    smp, ids = live_inputs(case, 128)
    live = dict(batch_size=32, threads=2, depth=3)
    drawn = []
    orig = smp.batch

    def recording(targets, mode, **kw):
        out = orig(targets, mode, **kw)
        drawn.append((np.array(targets), kw["counter"], out[0]["node_ids"].clone(), out[1]["node_ids"].clone(), out[3].clone()))
        return out
    smp.batch = recording

    def same(a, b):
        return np.array_equal(a[0], b[0]) and a[1] == b[1] and all(torch.equal(x, y) for x, y in zip(a[2:], b[2:]))
    eng_a = make_engine(case, dtype="bf16", **DROP)
    tr_a = Trainer(eng_a, **KW)
    tr_a.run_live(smp, ids, steps=6, **live)
    one_call, drawn[:] = list(drawn), []
    assert [d[1] for d in one_call] == [32 * i for i in range(6)] and tr_a.pipeline_step == 6
    eng_b = make_engine(case, dtype="bf16", **DROP)
    tr_b = Trainer(eng_b, **KW)
    tr_b.run_live(smp, ids, steps=3, **live)
    tr_b.run_live(smp, ids, steps=3, first_step=3, **live)
    two_calls, drawn[:] = list(drawn), []
    assert tr_b.pipeline_step == 6 and all(same(a, b) for a, b in zip(one_call, two_calls))
    assert_same_state(state_of(eng_a), state_of(eng_b))
    assert tr_a.last_loss.item() == tr_b.last_loss.item()
    # the default: every call starts its streams at 0 again, as before the keyword existed
    eng_c = make_engine(case, dtype="bf16", **DROP)
    tr_c = Trainer(eng_c, **KW)
    tr_c.run_live(smp, ids, steps=3, **live)
    tr_c.run_live(smp, ids, steps=3, **live)
    assert [d[1] for d in drawn] == [0, 32, 64, 0, 32, 64] and all(same(a, b) for a, b in zip(drawn[:3], drawn[3:]))
    assert all(same(a, b) for a, b in zip(drawn[:3], one_call[:3])) and not same(drawn[3], one_call[3])
    assert not torch.equal(eng_c.params, eng_a.params)


@pytest.mark.parametrize("name", ["m1", "m4"])
def test_resumed_curve_matches_the_reference(name, tmp_path):
    """The reference's six optimizer steps (injected NFR draws, dropout off: the fixture's) with a save after step 2 and a load into a fresh
    engine: losses 3 - 5, their gradient norms and the final parameters within test_clip_adamw_curve_matches_reference's bounds."""
    from pmgt_amd import io as pio
    from pmgt_amd.trainer import Trainer
    case = gu.model_case(name)
    gold = case["gold"]
    batch = dev_batch(case["batch"])
    hyper = dict(lr=1e-3, weight_decay=1e-2, max_grad_norm=5.0)
    assert len(gold["opt_losses"]) == 6 and not np.isnan(gold["opt_losses"]).any()

    def steps(eng, which):
        for s in which:
            inj, _ = inject_for(case, "opt_", f"_{s}")
            out = eng.pretrain_step(batch, training=True, backward=True, nfr_inject=inj)
            eng.optimizer_step(**hyper)
            np.testing.assert_allclose(out["loss"].item(), gold["opt_losses"][s], rtol=2e-4)
            np.testing.assert_allclose(eng.grad_norm().item(), gold["opt_gradnorms"][s], rtol=1e-3)
    eng = make_engine(case)
    steps(eng, range(3))
    pio.save_training_checkpoint(eng, Trainer(eng, **hyper), tmp_path / "s3.ckpt")
    eng2 = fresh_engine(case, "fp32", seed=1)
    pio.load_training_checkpoint(eng2, Trainer(eng2, **hyper), tmp_path / "s3.ckpt")
    assert int(eng2.opt_step.item()) == 3
    steps(eng2, range(3, 6))
    for k, v in eng2.named_views().items():
        gu.check_stored(gold, "final/" + k, v.cpu().numpy(), 2e-3, 2e-5)


# ======================================================================================================== fit, on a small synthetic graph
FIT_N, FIT_S, FIT_B = 200, 16, 48
FIT_CFG = dict(hidden_size=64, num_hidden_layers=2, num_attention_heads=4, intermediate_size=64, beta=0.5, **DROP)
BEST_NAME = re.compile(r"^epoch=\d\d-(loss|auc)=\d+\.\d{4}\.ckpt$")


class Stop(Exception):
    pass


def fit_world(world_size=1, **trainer_kw):
    """Engine (fp32, dropout on) + trainer + sampler + the train / valid split of a 200-node graph: 160 train ids = 3 batches of 48 and a
    remainder of 16 per epoch on one rank."""
    from pmgt_amd.configuration_pmgt import PMGTConfig
    from pmgt_amd.datasets import MCNSampler, train_valid_split
    from pmgt_amd.engine import Engine
    from pmgt_amd.graph import synthetic_graph
    from pmgt_amd.trainer import Trainer
    ocfg = po.default_cfg(**FIT_CFG)
    eng = Engine(PMGTConfig(**FIT_CFG), dtype="fp32", device="cuda:0", seed=0)
    eng.load_params(po.synth_params(ocfg, 3))
    eng.set_tables(*[t.numpy() for t in po.synth_tables(FIT_N, ocfg["feat_hidden_sizes"], 4)])
    smp = MCNSampler(synthetic_graph(FIT_N, 1000, seed=3), FIT_S - 1)
    train_ids, valid_ids = train_valid_split(FIT_N, 0.2, seed=1)
    tr = Trainer(eng, lr=1e-3, weight_decay=1e-2, max_grad_norm=5.0, scheduler_type="linear", num_warmup_steps=2, num_training_steps=16,
                 world_size=world_size, **trainer_kw)
    return eng, tr, smp, train_ids, valid_ids


def stop_after(global_step):
    def log(ev):
        if ev["event"] == "train" and ev["global_step"] == global_step:
            raise Stop()
    return log


@pytest.mark.parametrize("criterion", ["loss", "auc"])
def test_fit_resumed_in_the_middle_of_an_epoch_equals_the_uninterrupted_run(criterion, tmp_path):
    from pmgt_amd import io as pio
    from pmgt_amd.trainer import fit
    args = dict(batch_size=FIT_B, max_epochs=3, early_criterion=criterion, patience=5, seed=5, threads=2, valid_batch_size=32)
    eng_a, tr_a, smp, train_ids, valid_ids = fit_world()
    events = []
    res_a = fit(tr_a, eng_a, smp, train_ids, valid_ids, ckpt_dir=str(tmp_path / "a"), log=events.append, **args)
    assert res_a["epochs_run"] == 3 and not res_a["stopped_early"] and len(res_a["history"]) == 3
    assert int(eng_a.opt_step.item()) == 12 and tr_a.pipeline_step == 12          # 3 full batches + the remainder, per epoch
    assert [e["event"] for e in events] == ["train", "train", "valid"] * 3
    # (b): killed after the 6th optimizer step = the second batch of epoch 1; a fresh engine and trainer pick last.ckpt up
    eng_b, tr_b, smp_b, _, _ = fit_world()
    with pytest.raises(Stop):
        fit(tr_b, eng_b, smp_b, train_ids, valid_ids, ckpt_dir=str(tmp_path / "b"), save_every_n_steps=1, log=stop_after(6), **args)
    ck = pio.read_checkpoint(str(tmp_path / "b" / "last.ckpt"))
    assert ck["global_step"] == 6 and ck["epoch"] == 1 and ck["pmgt_amd"]["fit"]["batches_done"] == 2 and ck["pmgt_amd"]["pipeline_step"] == 6
    del eng_b, tr_b
    eng_c, tr_c, smp_c, _, _ = fit_world()
    eng_c.params.zero_()
    res_c = fit(tr_c, eng_c, smp_c, train_ids, valid_ids, ckpt_dir=str(tmp_path / "b"), save_every_n_steps=1, resume_from="last", **args)
    assert res_c["history"] == res_a["history"]                                   # per-epoch validation metrics, exactly
    assert os.path.basename(res_c["best_model_path"]) == os.path.basename(res_a["best_model_path"])
    assert res_c["best_model_score"] == res_a["best_model_score"] and res_c["epochs_run"] == 3 and not res_c["stopped_early"]
    assert_same_state(state_of(eng_a), state_of(eng_c))
    for d, res in (("a", res_a), ("b", res_c)):
        files = sorted(os.listdir(tmp_path / d))
        assert len(files) == 2 and "last.ckpt" in files, files                    # last + exactly one best, no temporary file
        best = [f for f in files if f != "last.ckpt"][0]
        assert BEST_NAME.match(best) and f"-{criterion}=" in best and best == os.path.basename(res["best_model_path"])
        monitor = "loss/val" if criterion == "loss" else "val/auc"
        scores = [h[monitor] for h in res["history"]]
        ep = int(np.argmin(scores) if criterion == "loss" else np.argmax(scores))
        assert best == f"epoch={ep:02d}-{criterion}={scores[ep]:.4f}.ckpt" and res["best_model_score"] == scores[ep]
    # a finished run resumed again has nothing left to do
    res_d = fit(tr_c, eng_c, smp_c, train_ids, valid_ids, ckpt_dir=str(tmp_path / "b"), resume_from="last", **args)
    assert res_d["history"] == res_a["history"] and int(eng_c.opt_step.item()) == 12


def test_fit_stops_early_on_a_scripted_metric(tmp_path, monkeypatch):
    from pmgt_amd import fit_loop, trainer as T
    script = iter([{"loss/val": 0.50, "val/auc": 0.6}, {"loss/val": 0.40, "val/auc": 0.7}, {"loss/val": 0.40, "val/auc": 0.8},
                   {"loss/val": 0.10, "val/auc": 0.9}])
    monkeypatch.setattr(fit_loop, "evaluate", lambda *a, **k: next(script))      # where fit looks it up
    eng, tr, smp, train_ids, valid_ids = fit_world()
    res = T.fit(tr, eng, smp, train_ids, valid_ids, batch_size=FIT_B, max_epochs=4, early_criterion="loss", patience=1,
                ckpt_dir=str(tmp_path), seed=5, threads=2)
    assert res["stopped_early"] and res["epochs_run"] == 3 and len(res["history"]) == 3       # the tie of epoch 2 is no improvement
    assert res["best_model_score"] == 0.40 and os.path.basename(res["best_model_path"]) == "epoch=01-loss=0.4000.ckpt"
    assert sorted(os.listdir(tmp_path)) == ["epoch=01-loss=0.4000.ckpt", "last.ckpt"]
    assert int(eng.opt_step.item()) == 12
    # a stopped run stays stopped when it is resumed
    again = T.fit(tr, eng, smp, train_ids, valid_ids, batch_size=FIT_B, max_epochs=4, early_criterion="loss", patience=1,
                  ckpt_dir=str(tmp_path), seed=5, threads=2, resume_from="last")
    assert again["stopped_early"] and again["epochs_run"] == 3 and int(eng.opt_step.item()) == 12


def test_fit_steps_an_unfinished_accumulation_window_at_the_end_of_an_epoch(tmp_path):
    """4 micro-batches per epoch under accumulation 3: one full window and one of a single micro-batch, stepped at the epoch's end."""
    from pmgt_amd.trainer import fit
    eng, tr, smp, train_ids, valid_ids = fit_world(accumulate_grad_batches=3)
    res = fit(tr, eng, smp, train_ids, valid_ids, batch_size=FIT_B, max_epochs=2, patience=5, ckpt_dir=str(tmp_path), seed=5, threads=2,
              save_every_n_steps=1)
    assert res["epochs_run"] == 2 and int(eng.opt_step.item()) == 4 and tr.pipeline_step == 8 and tr._micro == 0


# ---- two ranks on this GPU over gloo (as tests/test_dp_gpu.py) ------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fit_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from pmgt_amd import io as pio
    from pmgt_amd.trainer import fit
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        real_save = pio.atomic_save

        def marking_save(obj, path):
            open(os.path.join(out_dir, f"wrote_rank{rank}"), "w").close()
            real_save(obj, path)
        pio.atomic_save = marking_save
        args = dict(batch_size=32, max_epochs=2, early_criterion="auc", patience=5, seed=5, threads=2, valid_batch_size=16)

        def world_():
            eng, tr, smp, train_ids, valid_ids = fit_world(world_size=world)
            if rank == 1:
                eng.params.mul_(1.5)
            tr.broadcast_parameters()
            return eng, tr, smp, train_ids, valid_ids
        eng, tr, smp, train_ids, valid_ids = world_()            # 80 ids per rank: 2 batches of 32 and a remainder of 16 per epoch
        full = fit(tr, eng, smp, train_ids, valid_ids, ckpt_dir=os.path.join(out_dir, "full"), **args)
        torch.cuda.synchronize()
        torch.save({"state": {k: v.cpu() for k, v in state_of(eng).items()}, "history": full["history"],
                    "best": os.path.basename(full["best_model_path"])}, os.path.join(out_dir, f"full{rank}.pt"))
        eng, tr, smp, _, _ = world_()
        try:
            fit(tr, eng, smp, train_ids, valid_ids, ckpt_dir=os.path.join(out_dir, "res"), save_every_n_steps=1, log=stop_after(4), **args)
            raise AssertionError("the injected stop did not fire")
        except Stop:
            pass
        dist.barrier()                                            # rank 0 has written last.ckpt before anybody reads it
        eng, tr, smp, _, _ = world_()
        eng.params.zero_()
        res = fit(tr, eng, smp, train_ids, valid_ids, ckpt_dir=os.path.join(out_dir, "res"), save_every_n_steps=1, resume_from="last", **args)
        torch.cuda.synchronize()
        torch.save({"state": {k: v.cpu() for k, v in state_of(eng).items()}, "history": res["history"],
                    "best": os.path.basename(res["best_model_path"])}, os.path.join(out_dir, f"res{rank}.pt"))
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_two_ranks_resume_to_identical_replicas_and_only_rank_0_writes(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_fit_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    got = {k: torch.load(tmp_path / f"{k}.pt", weights_only=False) for k in ("full0", "full1", "res0", "res1")}
    assert os.path.exists(tmp_path / "wrote_rank0") and not os.path.exists(tmp_path / "wrote_rank1")
    ref = got["full0"]
    assert int(ref["state"]["opt_step"]) == 6 and len(ref["history"]) == 2
    for k in ("full1", "res0", "res1"):
        assert_same_state(ref["state"], got[k]["state"])
        assert got[k]["history"] == ref["history"] and got[k]["best"] == ref["best"]
    for d in ("full", "res"):
        files = sorted(os.listdir(tmp_path / d))
        assert len(files) == 2 and "last.ckpt" in files and ref["best"] in files and BEST_NAME.match(ref["best"]), files
