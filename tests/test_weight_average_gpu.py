"""Weight averaging from the trainer up (pmgt_amd/averaging.py, Trainer(weight_average=...), Trainer.averaged_weights(), the checkpoint
block, fit(swa_epoch_start=...)): the golden model m1 (B = 4) for the step-level tests, the 200-node graph of tests/test_resume_gpu.py
for fit.

Bounds.  Bit-exact throughout.  The average is replayed on the host from parameter snapshots with the numpy restatement
(tests/weight_average_util.py: two fp32 products and one fp32 sum, the kernel's contract); parameters, moments and counters of an
averaging trainer against a trainer without averaging, a captured run against an eager one and a resumed run against the uninterrupted one
are compared with torch.equal on the raw words; validation metrics on the averaged weights against `evaluate` of a second engine loaded
with the hand-computed average with == (the same kernels on the same bits).  Dropout is on wherever the fixture allows, so a step that
ran once too often or too seldom shows."""
import math
import os

import numpy as np
import pytest
import torch

from tests import golden_util as gu
from tests import weight_average_util as wu
from tests.test_engine_gpu import dev_batch, make_engine
from tests.test_guarded_step_gpu import poison_table, poisoned_step, same_bits
from tests.test_resume_gpu import DROP, KW, Stop, assert_same_state, fit_world, fresh_engine, live_inputs, state_of, stop_after

pytestmark = pytest.mark.gpu

EMA = dict(mode="ema", decay=0.3, warmup=True)        # the warm-up ramp 0.1, 0.18, 0.25 reaches 0.3 at the fourth update: both branches


@pytest.fixture(autouse=True)
def _no_graph_left_behind():
    """Captured steps are destroyed here, with the GPU idle (see tests/test_lr_schedule_gpu.py)."""
    yield
    import gc
    torch.cuda.synchronize()
    gc.collect()


def trainer_on(case, dtype="bf16", drop=DROP, **kw):
    from pmgt_amd.trainer import Trainer
    eng = make_engine(case, dtype=dtype, **drop)
    return eng, Trainer(eng, **dict(KW, **kw))


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def bits_equal(t, arr):
    return np.array_equal(host(t).view(np.uint32), np.asarray(arr, dtype=np.float32).view(np.uint32))


def test_eager_ema_follows_the_host_replay_and_changes_no_bit_of_the_run():
    case = gu.model_case("m1")
    batch = dev_batch(case["batch"])
    eng, tr = trainer_on(case, weight_average=EMA)
    eng_plain, tr_plain = trainer_on(case)
    wa = tr.weight_average
    assert wa.mode == "ema" and wa.avg.data_ptr() != eng.params.data_ptr() and torch.equal(wa.avg, eng.params) and wa.count() == 0
    start, snaps = host(eng.params), []
    for _ in range(6):
        tr.train_step(batch)
        snaps.append(host(eng.params))
        tr_plain.train_step(batch)
    assert bits_equal(wa.avg, wu.ema_replay_np(start, snaps, EMA["decay"], EMA["warmup"]))
    st = wa.device_state()
    assert wa.count() == 6 and st["skipped"] == 0 and st["w_old"] == float(np.float32(0.3)) and st["w_new"] == float(np.float32(1.0 - 0.3))
    assert_same_state(state_of(eng), state_of(eng_plain))
    assert not torch.equal(wa.avg, eng.params) and bool(torch.isfinite(wa.avg).all())
    # "swa" mode: the step does nothing extra; update() is swa_step
    eng_s, tr_s = trainer_on(case, weight_average=dict(mode="swa"))
    first = host(eng_s.params)
    tr_s.train_step(batch)
    assert bits_equal(tr_s.weight_average.avg, first) and tr_s.weight_average.state is None
    tr_s.weight_average.update()
    assert tr_s.weight_average.count() == 2 and bits_equal(tr_s.weight_average.avg, wu.swa_step_np(first, host(eng_s.params), 2))
    eng_q, tr_q = trainer_on(case)
    tr_q.train_step(batch)
    assert_same_state(state_of(eng_s), state_of(eng_q))


@pytest.mark.parametrize("guard", [dict(), dict(step_log=4, nonfinite="skip")], ids=["plain", "guarded"])
def test_captured_step_equals_eager_steps(guard):
    """capture_step (2 eager warm-up steps) + 5 replays against 7 eager steps: parameters, moments, counters, average and its count."""
    case = gu.model_case("m1")
    batch = dev_batch(case["batch"])
    eng_e, tr_e = trainer_on(case, weight_average=EMA, **guard)
    for _ in range(7):
        tr_e.train_step(batch)
    eng_c, tr_c = trainer_on(case, weight_average=EMA, **guard)
    replay = tr_c.capture_step(batch, warmup=2)
    assert any(t is tr_c.weight_average.avg for t in replay.keep) and any(t is tr_c.weight_average.state for t in replay.keep)
    assert tr_c.weight_average.count() == 2                    # the recording itself applied nothing
    for _ in range(5):
        replay()
    assert_same_state(state_of(eng_e), state_of(eng_c))
    assert same_bits(tr_e.weight_average.avg, tr_c.weight_average.avg)
    assert tr_e.weight_average.count() == tr_c.weight_average.count() == 7
    assert not torch.equal(tr_c.weight_average.avg, eng_c.params)
    if guard:
        assert eng_c.step_counters() == eng_e.step_counters() == {"attempts": 7, "skipped": 0, "skipped_in_a_row": 0}
    # the averaging settings are part of what a captured step is keyed on
    from pmgt_amd.trainer import Trainer
    plain = Trainer(eng_c, **dict(KW, **guard))
    assert tr_c._capture_key() != plain._capture_key() and plain._capture_key() == plain._hyper_key()
    assert tr_c._capture_key()[:-1] == tr_c._hyper_key() and tr_c._capture_key()[-1] == ("weight_average", "ema", 0.3, True)


def test_a_skipped_step_is_not_averaged_in_eager_and_replayed():
    case = gu.model_case("m1")
    batch = dev_batch(case["batch"])
    no_drop = dict(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    # eager: the Inf goes into the gradient buffer between backward and optimizer, as tests/test_guarded_step_gpu.py does
    eng, tr = trainer_on(case, drop=no_drop, weight_average=EMA, nonfinite="skip", step_log=4)
    wa = tr.weight_average
    start = host(eng.params)
    tr.train_step(batch)
    p1, a1 = host(eng.params), host(wa.avg)
    assert wa.count() == 1 and bits_equal(wa.avg, wu.ema_replay_np(start, [p1], 0.3, True))
    poisoned_step(tr, batch)
    assert eng.was_skipped().item() == 1.0 and wa.count() == 1 and wa.device_state()["skipped"] == 1
    assert bits_equal(wa.avg, a1) and bits_equal(eng.params, p1)
    tr.train_step(batch)
    p2 = host(eng.params)
    assert wa.count() == 2 and wa.device_state()["skipped"] == 0 and not np.array_equal(p1, p2)
    assert bits_equal(wa.avg, wu.ema_replay_np(start, [p1, p2], 0.3, True))
    assert eng.step_counters() == {"attempts": 3, "skipped": 1, "skipped_in_a_row": 0}
    # replayed: a frozen table row at inf makes the replay's gradient norm non-finite
    eng, tr = trainer_on(case, drop=no_drop, weight_average=EMA, nonfinite="skip", step_log=4)
    wa = tr.weight_average
    replay = tr.capture_step(batch, warmup=2)
    replay()
    p3, a3 = host(eng.params), host(wa.avg)
    assert wa.count() == 3
    restore = poison_table(eng, batch)
    replay()
    assert wa.count() == 3 and wa.device_state()["skipped"] == 1 and bits_equal(wa.avg, a3) and bits_equal(eng.params, p3)
    restore()
    replay()
    p4 = host(eng.params)
    assert wa.count() == 4 and not np.array_equal(p3, p4)
    assert bits_equal(wa.avg, wu.ema_replay_np(a3, [p4], 0.3, True, first_n=3))
    assert eng.step_counters() == {"attempts": 5, "skipped": 1, "skipped_in_a_row": 0}


def averaged_world():
    """m1 trainer with an EMA average, a step captured (2 warm-up steps), and its twin for forward work on other weights."""
    case = gu.model_case("m1")
    batch = dev_batch(case["batch"])
    eng, tr = trainer_on(case, weight_average=EMA)
    replay = tr.capture_step(batch, warmup=2)
    smp, ids = live_inputs(case, 24)
    return case, batch, eng, tr, replay, smp, ids


def test_averaged_weights_context():
    from pmgt_amd.trainer import evaluate
    case, batch, eng, tr, replay, smp, ids = averaged_world()
    wa = tr.weight_average
    p0, a0 = eng.params.clone(), wa.avg.clone()
    ptrs = (eng.params.data_ptr(), wa.avg.data_ptr())
    assert not torch.equal(p0, a0)
    ev = dict(batch_size=8, threads=2, seed=1)
    raw = evaluate(eng, smp, ids, **ev)
    with tr.averaged_weights() as inside:
        assert inside is wa and same_bits(eng.params, a0) and same_bits(wa.avg, p0)
        got = evaluate(eng, smp, ids, **ev)
        for call in (lambda: tr.train_step(batch), lambda: tr.training_step(batch), tr.optimizer_step, lambda: tr.capture_step(batch)):
            with pytest.raises(RuntimeError, match=r"averaged_weights\(\)"):
                call()
        with pytest.raises(RuntimeError, match="entered twice"):
            with tr.averaged_weights():
                pass
        assert same_bits(eng.params, a0)                     # the refused calls moved nothing
    assert same_bits(eng.params, p0) and same_bits(wa.avg, a0) and (eng.params.data_ptr(), wa.avg.data_ptr()) == ptrs
    eng2 = make_engine(case, dtype="bf16", **DROP)
    eng2.params.copy_(a0)
    assert got == evaluate(eng2, smp, ids, **ev) and got != raw
    with pytest.raises(KeyError, match="boom"):
        with tr.averaged_weights():
            raise KeyError("boom")
    assert same_bits(eng.params, p0) and same_bits(wa.avg, a0) and not tr._averaged
    # the step captured BEFORE the context replays correctly AFTER it: the swap moved contents, not pointers
    replay()
    eng_t, tr_t = trainer_on(case, weight_average=EMA)
    for _ in range(3):
        tr_t.train_step(batch)
    assert_same_state(state_of(eng), state_of(eng_t))
    assert same_bits(wa.avg, tr_t.weight_average.avg) and wa.count() == 3
    from pmgt_amd.trainer import Trainer
    with pytest.raises(RuntimeError, match="keeps no weight average"):
        with Trainer(eng_t, **KW).averaged_weights():
            pass


def test_export_inside_the_context_exports_the_average():
    from pmgt_amd.trainer import export_embeddings
    case, batch, eng, tr, replay, smp, ids = averaged_world()
    a0 = tr.weight_average.avg.clone()
    n = 40
    raw = export_embeddings(eng, smp, n, batch_size=16, threads=2)
    with tr.averaged_weights():
        got = export_embeddings(eng, smp, n, batch_size=16, threads=2)
    eng2 = make_engine(case, dtype="bf16", **DROP)
    eng2.params.copy_(a0)
    want = export_embeddings(eng2, smp, n, batch_size=16, threads=2)
    assert got.shape == (n, eng.config.hidden_size) and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert not np.array_equal(got, raw)


def test_checkpoint_block_loads_in_place_and_the_four_cases():
    from pmgt_amd.trainer import Trainer
    case = gu.model_case("m1")
    batch = dev_batch(case["batch"])
    eng, tr = trainer_on(case, weight_average=EMA)
    for _ in range(3):
        tr.train_step(batch)
    sd = tr.state_dict()
    block = sd["weight_average"]
    assert (block["mode"], block["decay"], block["warmup"], block["n_upd"]) == ("ema", 0.3, True, 3) and block["average"].device.type == "cpu"
    assert "weight_average" not in Trainer(eng, **KW).state_dict()
    avg3 = tr.weight_average.avg.clone()
    # continue 2 steps, load in place (a captured step alive), continue again: the same bits
    replay = tr.capture_step(batch, warmup=0)
    ptr = tr.weight_average.avg.data_ptr()
    replay(), replay()
    want, want_avg = state_of(eng), tr.weight_average.avg.clone()
    tr.load_state_dict(sd)
    assert tr.weight_average.avg.data_ptr() == ptr and same_bits(tr.weight_average.avg, avg3) and tr.weight_average.count() == 3
    replay(), replay()
    assert_same_state(want, state_of(eng))
    assert same_bits(tr.weight_average.avg, want_avg) and tr.weight_average.count() == 5
    # into a fresh engine
    eng_f = fresh_engine(case, "bf16", seed=4, **DROP)
    tr_f = Trainer(eng_f, weight_average=EMA, **KW)
    tr_f.load_state_dict(sd)
    tr_f.train_step(batch), tr_f.train_step(batch)
    assert_same_state(want, state_of(eng_f))
    assert same_bits(tr_f.weight_average.avg, want_avg)
    # the file has a block, the trainer does not average
    eng_n = fresh_engine(case, "bf16", **DROP)
    with pytest.raises(ValueError, match="weight_average: checkpoint set, trainer None"):
        Trainer(eng_n, **KW).load_state_dict(sd)
    assert float(eng_n.params.abs().max()) == 0.0                                  # refused before anything was written
    Trainer(eng_n, **KW).load_state_dict(sd, strict=False)
    assert same_bits(eng_n.params, sd["engine"]["params"].cuda())
    # the file has none, the trainer averages
    bare = {k: v for k, v in sd.items() if k != "weight_average"}
    eng_m = fresh_engine(case, "bf16", **DROP)
    tr_m = Trainer(eng_m, weight_average=EMA, **KW)
    with pytest.raises(ValueError, match="weight_average: checkpoint None, trainer set"):
        tr_m.load_state_dict(bare)
    assert float(eng_m.params.abs().max()) == 0.0
    tr_m.weight_average.state[0] = 9
    tr_m.load_state_dict(bare, strict=False)
    assert same_bits(tr_m.weight_average.avg, eng_m.params) and tr_m.weight_average.count() == 0 and float(eng_m.params.abs().max()) > 0.0
    # other settings: a hyper-parameter mismatch like the others
    eng_o = fresh_engine(case, "bf16", **DROP)
    tr_o = Trainer(eng_o, weight_average=dict(mode="ema", decay=0.5, warmup=True), **KW)
    with pytest.raises(ValueError, match="weight_average.decay: checkpoint 0.3, trainer 0.5"):
        tr_o.load_state_dict(sd)
    assert float(eng_o.params.abs().max()) == 0.0
    tr_o.load_state_dict(sd, strict=False)
    assert same_bits(tr_o.weight_average.avg, avg3) and tr_o.weight_average.count() == 3 and tr_o.weight_average.decay == 0.5


# ======================================================================================================== fit, on the 200-node graph
FIT = dict(batch_size=48, patience=5, seed=5, threads=2, valid_batch_size=32)


def test_fit_swa_validates_on_the_running_mean_and_resumes_bit_identically(tmp_path):
    from pmgt_amd import io as pio
    from pmgt_amd.trainer import evaluate, fit
    eng, tr, smp, train_ids, valid_ids = fit_world()
    ends = []                                               # raw parameters at the end of every epoch (the "valid" event follows the swap back)
    fit_args = dict(max_epochs=4, swa_epoch_start=2, **FIT)
    res = fit(tr, eng, smp, train_ids, valid_ids, ckpt_dir=str(tmp_path / "a"),
              log=lambda ev: ends.append(host(eng.params)) if ev["event"] == "valid" else None, **fit_args)
    assert res["epochs_run"] == 4 and len(ends) == 4 and tr.weight_average.mode == "swa" and tr.weight_average.count() == 4
    assert bits_equal(eng.params, ends[3]) and not tr._averaged
    # by hand: swa_init at the start of epoch 1 (= the end of epoch 0), one swa_step before each of the validations of epochs 1, 2, 3
    eng2, _, smp2, _, _ = fit_world()
    avg = ends[0]
    ev = dict(batch_size=FIT["valid_batch_size"], threads=FIT["threads"], seed=FIT["seed"])
    eng2.params.copy_(torch.from_numpy(ends[0]))
    assert res["history"][0] == dict(epoch=0, **evaluate(eng2, smp2, valid_ids, **ev))          # before the start epoch: the raw weights
    for e, models_num in ((1, 2), (2, 3), (3, 4)):
        avg = wu.swa_step_np(avg, ends[e], models_num)
        eng2.params.copy_(torch.from_numpy(avg))
        assert res["history"][e] == dict(epoch=e, **evaluate(eng2, smp2, valid_ids, **ev)), e
        eng2.params.copy_(torch.from_numpy(ends[e]))
        assert res["history"][e] != dict(epoch=e, **evaluate(eng2, smp2, valid_ids, **ev)), e   # the test can tell the two apart
    assert bits_equal(tr.weight_average.avg, avg)
    ck = pio.read_checkpoint(str(tmp_path / "a" / "last.ckpt"))
    key = "StochasticWeightAveraging{'swa_epoch_start': 2, 'annealing_strategy': 'cos'}"
    model = ck["callbacks"][key]["average_model"]
    assert model["models_num"] == 4 and ck["pmgt_amd"]["weight_average"]["models_num"] == 4 and ck["pmgt_amd"]["weight_average"]["mode"] == "swa"
    assert np.array_equal(ck["pmgt_amd"]["weight_average"]["average"].numpy().view(np.uint32), avg.view(np.uint32))
    e0 = eng.entries[0]
    assert torch.equal(model["net." + e0["name"]].reshape(-1), ck["pmgt_amd"]["weight_average"]["average"][e0["offset"]: e0["offset"] + e0["numel"]])
    assert np.array_equal(ck["state_dict"]["net." + e0["name"]].numpy().reshape(-1), ends[3][e0["offset"]: e0["offset"] + e0["numel"]])   # raw weights
    # interrupted after the second validation (epochs 0 and 1 done: the file carries models_num = 2), resumed in a fresh world
    eng_b, tr_b, smp_b, _, _ = fit_world()
    seen = []

    def stop_after_two_validations(event):
        if event["event"] == "valid":
            seen.append(1)
            if len(seen) == 2:
                raise Stop()
    with pytest.raises(Stop):
        fit(tr_b, eng_b, smp_b, train_ids, valid_ids, ckpt_dir=str(tmp_path / "b"), log=stop_after_two_validations, **fit_args)
    assert pio.read_checkpoint(str(tmp_path / "b" / "last.ckpt"))["pmgt_amd"]["weight_average"]["models_num"] == 2
    del eng_b, tr_b
    eng_c, tr_c, smp_c, _, _ = fit_world()
    eng_c.params.zero_()
    res_c = fit(tr_c, eng_c, smp_c, train_ids, valid_ids, ckpt_dir=str(tmp_path / "b"), resume_from="last", **fit_args)
    assert res_c["history"] == res["history"] and res_c["best_model_score"] == res["best_model_score"]
    assert os.path.basename(res_c["best_model_path"]) == os.path.basename(res["best_model_path"]) and res_c["epochs_run"] == 4
    assert_same_state(state_of(eng), state_of(eng_c))
    assert same_bits(tr.weight_average.avg, tr_c.weight_average.avg) and tr_c.weight_average.count() == 4
    assert sorted(os.listdir(tmp_path / "a")) == sorted(os.listdir(tmp_path / "b")) and len(os.listdir(tmp_path / "b")) == 2
    # refusals
    with pytest.raises(ValueError, match="swa_epoch_start should be a >0 integer or a float between 0 and 1."):
        fit(tr_c, eng_c, smp_c, train_ids, valid_ids, ckpt_dir=str(tmp_path / "x"), max_epochs=4, swa_epoch_start=0, **FIT)
    eng_e, tr_e, smp_e, _, _ = fit_world(weight_average=EMA)
    with pytest.raises(ValueError, match="'swa' mode"):
        fit(tr_e, eng_e, smp_e, train_ids, valid_ids, ckpt_dir=str(tmp_path / "x"), max_epochs=4, swa_epoch_start=2, **FIT)


def test_fit_ema_validates_on_the_average_and_resumes_inside_an_epoch(tmp_path):
    from pmgt_amd import io as pio
    from pmgt_amd.trainer import evaluate, fit
    args = dict(max_epochs=2, save_every_n_steps=1, **FIT)
    eng, tr, smp, train_ids, valid_ids = fit_world(weight_average=EMA)
    seen = []
    res = fit(tr, eng, smp, train_ids, valid_ids, ckpt_dir=str(tmp_path / "a"),
              log=lambda ev: seen.append((host(eng.params), host(tr.weight_average.avg))) if ev["event"] == "valid" else None, **args)
    assert int(eng.opt_step.item()) == 8 and tr.weight_average.count() == 8 and len(res["history"]) == 2
    eng2, _, smp2, _, _ = fit_world()
    ev = dict(batch_size=FIT["valid_batch_size"], threads=FIT["threads"], seed=FIT["seed"])
    for e, (raw, avg) in enumerate(seen):                   # from the first epoch on, the metric is the average's
        eng2.params.copy_(torch.from_numpy(avg))
        assert res["history"][e] == dict(epoch=e, **evaluate(eng2, smp2, valid_ids, **ev))
        assert not np.array_equal(raw, avg)
    eng_b, tr_b, smp_b, _, _ = fit_world(weight_average=EMA)
    with pytest.raises(Stop):
        fit(tr_b, eng_b, smp_b, train_ids, valid_ids, ckpt_dir=str(tmp_path / "b"), log=stop_after(6), **args)
    ck = pio.read_checkpoint(str(tmp_path / "b" / "last.ckpt"))
    assert ck["global_step"] == 6 and ck["pmgt_amd"]["fit"]["batches_done"] == 2 and ck["pmgt_amd"]["weight_average"]["n_upd"] == 6
    assert pio._callback(ck["callbacks"], "StochasticWeightAveraging")["average_model"]["n_upd"] == 6
    del eng_b, tr_b
    eng_c, tr_c, smp_c, _, _ = fit_world(weight_average=EMA)
    eng_c.params.zero_()
    res_c = fit(tr_c, eng_c, smp_c, train_ids, valid_ids, ckpt_dir=str(tmp_path / "b"), resume_from="last", **args)
    assert res_c["history"] == res["history"] and res_c["best_model_score"] == res["best_model_score"]
    assert_same_state(state_of(eng), state_of(eng_c))
    assert same_bits(tr.weight_average.avg, tr_c.weight_average.avg) and tr_c.weight_average.count() == 8
    assert math.isfinite(res["history"][-1]["loss/val"])
