"""Host side of weight averaging (pmgt_amd/averaging.py, the weight_average block of pmgt_amd/io.py), no GPU: the decay series, the
start-epoch arithmetic of the reference's callback (pmgt/callbacks.py:54-58,91-93,136-137), the numpy restatement the GPU tests compare
the kernels with, and the checkpoint block with its four strict / non-strict load decisions (averaging.reconcile: the pure function
Trainer.load_state_dict asks; the trainer-level loads themselves need an engine and live in tests/test_weight_average_gpu.py).

Bounds.  The decay series and the epoch arithmetic are exact (==): one fp64 division, correctly rounded on both sides.  The restatement
against torch's mul_(1 - beta).add_(p, alpha=beta) on the CPU: torch may or may not fuse alpha * p into the add, so the two sides round
differently; each side rounds at most three times, each rounding at most 2^-24 relative of a term bounded by |avg| + |p| (the weights
are in [0, 1]), so |a - b| <= 6 * 2^-24 * (|avg| + |p|) < 2^-21 * (|avg| + |p|) per element."""
from fractions import Fraction

import numpy as np
import pytest
import torch

from pmgt_amd import averaging as av
from pmgt_amd import io as pio
from tests import weight_average_util as wu
from tests.test_checkpoint_state_cpu import make_entries, trainer_sd, weights_of

# (1 + n) / (10 + n) for n = 0 .. 40, written out
WARMUP_TABLE = ["1/10", "2/11", "3/12", "4/13", "5/14", "6/15", "7/16", "8/17", "9/18", "10/19", "11/20", "12/21", "13/22", "14/23", "15/24",
                "16/25", "17/26", "18/27", "19/28", "20/29", "21/30", "22/31", "23/32", "24/33", "25/34", "26/35", "27/36", "28/37", "29/38",
                "30/39", "31/40", "32/41", "33/42", "34/43", "35/44", "36/45", "37/46", "38/47", "39/48", "40/49", "41/50"]


def test_ema_decay_series():
    assert len(WARMUP_TABLE) == 41
    ramp = [float(Fraction(s)) for s in WARMUP_TABLE]                     # Fraction -> float is correctly rounded, as the division is
    assert ramp[0] == 0.1 and ramp[8] == 0.5 and ramp[40] == 0.82
    for n in range(41):
        # decay 0.999: the ramp stays below it over the whole table; decay 0.5: the ramp reaches it at n = 8 ((1 + 8) / (10 + 8))
        assert av.ema_decay(n, 0.999, True) == ramp[n] < 0.999
        assert av.ema_decay(n, 0.5, True) == (ramp[n] if n < 8 else 0.5)
        assert av.ema_decay(n, 0.999, False) == 0.999 and av.ema_decay(n, 0.5, False) == 0.5
    assert av.ema_decay(7, 0.5) < 0.5 == av.ema_decay(8, 0.5) == av.ema_decay(9, 0.5)
    # 0.999 is reached where (1 + n) / (10 + n) >= 0.999, i.e. n >= 8990
    assert av.ema_decay(8989, 0.999) == 8990 / 8999 < 0.999 and av.ema_decay(8990, 0.999) == 0.999 == av.ema_decay(10 ** 9, 0.999)
    assert av.ema_decay(0) == 0.1 and av.ema_decay(10 ** 6) == 0.999      # the defaults: decay 0.999, warm-up on
    w_old, w_new = av.ema_weights(3, 0.999, True)
    assert w_old.dtype == w_new.dtype == np.float32 and w_old == np.float32(4 / 13) and w_new == np.float32(1.0 - 4 / 13)
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            av.check_settings("ema", bad, True)
    with pytest.raises(ValueError, match="mode"):
        av.check_settings("mean", 0.9, True)


def test_swa_start_epoch_arithmetic_and_refusals():
    # ints: 1-based epoch -> 0-based, never below 0
    assert [av.swa_start_epoch(k, 10) for k in (1, 2, 3, 10, 25)] == [0, 1, 2, 9, 24]
    # floats: int(max_epochs * f) first, then the same step down
    assert av.swa_start_epoch(0.8, 10) == 7 and av.swa_start_epoch(0.5, 4) == 1 and av.swa_start_epoch(0.75, 4) == 2
    assert av.swa_start_epoch(0.0, 10) == 0 and av.swa_start_epoch(0.05, 10) == 0 and av.swa_start_epoch(1.0, 4) == 3
    assert av.swa_start_epoch(0.3, 10) == int(10 * 0.3) - 1 == 2          # truncation, not rounding
    msg = "swa_epoch_start should be a >0 integer or a float between 0 and 1."
    for bad in (0, -1, -0.1, 1.5, 2.0, "2", None, True):
        with pytest.raises(ValueError) as ei:
            av.swa_start_epoch(bad, 10)
        assert str(ei.value) == msg


@pytest.mark.parametrize("n", [1, 5, 257, 3073])
def test_restatement_against_torch_on_the_cpu(n):
    """Three consecutive swa_steps (models_num 2, 3, 4) as the reference writes them, against the restatement; and the restatement's own
    fixed points."""
    avg, p = wu.special_inputs(n, seed=n)
    t_avg = torch.from_numpy(avg.copy())
    mine = avg.copy()
    for models_num in (2, 3, 4):
        beta = 1.0 / models_num
        t_p = torch.from_numpy(p)
        bound = 2.0 ** -21 * (np.abs(mine).astype(np.float64) + np.abs(p).astype(np.float64))
        t_avg.mul_(1.0 - beta).add_(t_p, alpha=beta)                       # pmgt/utils/train.py:69
        mine = wu.swa_step_np(mine, p, models_num)
        diff = np.abs(t_avg.numpy().astype(np.float64) - mine.astype(np.float64))
        assert (diff <= bound).all(), (models_num, float(diff.max()))
        mine = t_avg.numpy().copy()                                        # each step judged from equal inputs
        p = (p * np.float32(1.25)).astype(np.float32)
    x = np.array([1.5, -0.0, 1e30, 3.0], dtype=np.float32)
    assert np.array_equal(wu.avg_apply_np(x, x, 0.5, 0.5).view(np.uint32), x.view(np.uint32))
    assert wu.avg_apply_np(np.float32([1.5]), np.float32([-1.5]), 0.5, 0.5)[0] == 0.0
    # three roundings, not two: a fused multiply-add would give another bit here
    a, q, wo, wn = np.float32(1.0000001), np.float32(3.0000002), np.float32(1 / 3), np.float32(1.0 - 1 / 3)
    assert wu.avg_apply_np([a], [q], wo, wn)[0] == np.float32(np.float32(a * wo) + np.float32(q * wn))
    # ema_replay_np states the series independently: it agrees with the package's
    snaps = [np.full(3, k, dtype=np.float32) for k in (1.0, 2.0, 4.0)]
    want = np.zeros(3, dtype=np.float32)
    for k, s in enumerate(snaps):
        want = wu.avg_apply_np(want, s, *av.ema_weights(k, 0.999, True))
    assert np.array_equal(wu.ema_replay_np(np.zeros(3), snaps, 0.999, True), want)


def block_for(n, mode="swa", count=3, decay=0.999, warmup=True, seed=5):
    g = torch.Generator().manual_seed(seed)
    return av.average_block({"mode": mode, "decay": decay, "warmup": warmup}, count, torch.randn(n, generator=g))


@pytest.mark.parametrize("mode", ["swa", "ema"])
def test_checkpoint_block_round_trip(mode, tmp_path):
    entries, n = make_entries()
    tsd = trainer_sd(entries, n)
    plain = pio.training_checkpoint(weights_of(entries, tsd["engine"]["params"]), entries, tsd, epoch=1)
    assert "weight_average" not in plain["pmgt_amd"] and plain["callbacks"] == {}            # without averaging: the file as it always was
    assert "weight_average" not in pio.training_state_from_checkpoint(plain, entries, n)
    block = block_for(n, mode, count=4)
    tsd["weight_average"] = block
    key = "StochasticWeightAveraging{'swa_epoch_start': 2, 'annealing_strategy': 'cos'}"
    ck = pio.training_checkpoint(weights_of(entries, tsd["engine"]["params"]), entries, tsd, epoch=1, swa_key=key,
                                 callbacks={"EarlyStopping{}": {"wait_count": 0}})
    assert set(plain) == set(ck) and set(ck["pmgt_amd"]) - set(plain["pmgt_amd"]) == {"weight_average"}
    pio.atomic_save(ck, tmp_path / "a.ckpt")
    got = pio.read_checkpoint(str(tmp_path / "a.ckpt"))
    count = "models_num" if mode == "swa" else "n_upd"
    pv = got["pmgt_amd"]["weight_average"]
    assert (pv["mode"], pv["decay"], pv["warmup"], pv[count]) == (mode, 0.999, True, 4) and torch.equal(pv["average"], block["average"])
    model = pio._callback(got["callbacks"], "StochasticWeightAveraging")["average_model"]     # the reference's on_save_checkpoint key
    assert key in got["callbacks"] and model[count] == 4 and len(model) == len(entries) + 1
    for e in entries:
        t = model["net." + e["name"]]
        assert tuple(t.shape) == tuple(e["shape"]) and torch.equal(t.reshape(-1), block["average"][e["offset"]: e["offset"] + e["numel"]])
    assert pio._callback(got["callbacks"], "EarlyStopping") == {"wait_count": 0}
    back = pio.training_state_from_checkpoint(got, entries, n)["weight_average"]
    assert av.block_count(back) == 4 and back["mode"] == mode and torch.equal(back["average"], block["average"])
    # the per-name tensors are views of the flat average: the file holds its storage once, and a reader gets it back shared
    flat = pv["average"].untyped_storage().data_ptr()
    assert all(model["net." + e["name"]].untyped_storage().data_ptr() == flat for e in entries)


def test_the_four_load_decisions():
    n = 40
    swa = {"mode": "swa", "decay": 0.999, "warmup": True}
    block = block_for(n, "swa")
    assert av.reconcile(None, None, True) == av.reconcile(None, None, False) == "none"
    assert av.reconcile(block, swa, True, n) == av.reconcile(block, swa, False, n) == "load"
    # a file without the block into a trainer that averages
    with pytest.raises(ValueError, match="no weight average.*weight_average: checkpoint None, trainer set"):
        av.reconcile(None, swa, True)
    assert av.reconcile(None, swa, False) == "reinit"
    # a file with the block into a trainer that does not
    with pytest.raises(ValueError, match="weight_average: checkpoint set, trainer None"):
        av.reconcile(block, None, True)
    assert av.reconcile(block, None, False) == "ignore"
    # mode, decay, warm-up: named like the other hyper-parameters
    ema = {"mode": "ema", "decay": 0.99, "warmup": False}
    eblock = block_for(n, "ema", decay=0.999, warmup=True)
    assert av.settings_mismatches(eblock, ema) == [("weight_average.decay", 0.999, 0.99), ("weight_average.warmup", True, False)]
    assert av.settings_mismatches(block, swa) == [] and av.settings_mismatches(None, swa) == [] and av.settings_mismatches(block, None) == []
    with pytest.raises(ValueError, match="weight_average.decay: checkpoint 0.999, trainer 0.99; weight_average.warmup: checkpoint True, trainer False"):
        av.reconcile(eblock, ema, True)
    assert av.reconcile(eblock, ema, False) == "load"                     # the tensors and the count, the trainer's settings
    with pytest.raises(ValueError, match="weight_average.mode: checkpoint 'swa', trainer 'ema'"):
        av.reconcile(block, ema, True)
    assert av.reconcile(block, ema, False) == "reinit"                    # a model count is not an update count
    with pytest.raises(ValueError, match=r"shape \(40,\), expected \(41,\)"):
        av.reconcile(block, swa, False, 41)
