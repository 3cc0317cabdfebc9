"""Weight averaging on the device: the running mean of the reference's StochasticWeightAveraging callback (pmgt/callbacks.py:44-381 over
swa_init / swa_step / swap_swa_params, pmgt/utils/train.py:39-85) and a per-step exponential average that lives inside a captured step.
The kernels are pmgt_amd/ops/weight_average.hip (include/pmgt_capi.h states the arithmetic and the device state); this module states the
decay series and the start-epoch arithmetic as pure host functions, the way pmgt_amd/schedule.py states the learning-rate schedule, and
owns the average buffer.

The engine, its captured steps and the nn.Parameter views address the flat parameter buffer by pointer, so the reference's
`p.data, avg = avg, p.data` is not available here: swap() exchanges the CONTENTS of the two buffers in place."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

MODES = ("swa", "ema")
SWA_EPOCH_START_MESSAGE = "swa_epoch_start should be a >0 integer or a float between 0 and 1."      # pmgt/callbacks.py:54


def ema_decay(n: int, decay: float = 0.999, warmup: bool = True) -> float:
    """The decay of the update that follows n applied updates, as a Python double: `decay`, or with warm-up
    min(decay, (1 + n) / (10 + n)) -- the first updates forget the initial weights quickly.  The device computes the same two fp64
    operations and rounds d and 1.0 - d to fp32 once each."""
    d = float(decay)
    if warmup:
        d = min(d, (1.0 + float(int(n))) / (10.0 + float(int(n))))
    return d


def ema_weights(n: int, decay: float = 0.999, warmup: bool = True):
    """(w_old, w_new) of that update as the fp32 values the device writes."""
    d = ema_decay(n, decay, warmup)
    return np.float32(d), np.float32(1.0 - d)


def swa_weights(models_num: int):
    """(w_old, w_new) of swa_step for the model count AFTER its increment: beta = 1.0 / models_num, mul_(1.0 - beta).add_(p, alpha=beta)
    (pmgt/utils/train.py:65-69), both formed in doubles and rounded to fp32 once."""
    beta = 1.0 / int(models_num)
    return np.float32(1.0 - beta), np.float32(beta)


def check_swa_epoch_start(swa_epoch_start) -> None:
    """The constructor check of the callback (pmgt/callbacks.py:54-58); anything but an int or a float is refused alike."""
    ok = isinstance(swa_epoch_start, (int, float)) and not isinstance(swa_epoch_start, bool)
    if ok and isinstance(swa_epoch_start, int):
        ok = swa_epoch_start >= 1
    elif ok:
        ok = 0 <= swa_epoch_start <= 1
    if not ok:
        raise ValueError(SWA_EPOCH_START_MESSAGE)


def swa_start_epoch(swa_epoch_start, max_epochs: int) -> int:
    """0-based epoch at whose start the average is initialised: a float becomes int(max_epochs * f) (on_fit_start,
    pmgt/callbacks.py:136-137), then max(start - 1, 0) (swa_start, pmgt/callbacks.py:91-93)."""
    check_swa_epoch_start(swa_epoch_start)
    start = int(int(max_epochs) * swa_epoch_start) if isinstance(swa_epoch_start, float) else int(swa_epoch_start)
    return max(start - 1, 0)


def check_settings(mode, decay, warmup) -> dict:
    if mode not in MODES:
        raise ValueError(f"weight averaging mode={mode!r}: expected one of {MODES}")
    if not 0.0 <= float(decay) < 1.0:
        raise ValueError(f"weight averaging decay={decay!r}: expected a value in [0, 1)")
    return {"mode": mode, "decay": float(decay), "warmup": bool(warmup)}


# ---- the checkpoint block: plain data, no engine -----------------------------------------------------------------------------
def average_block(settings: dict, count: int, avg) -> dict:
    """The `weight_average` block of Trainer.state_dict(): the settings, the count (models_num in "swa" mode, n_upd in "ema" mode) and the
    flat average (a CPU tensor)."""
    key = "models_num" if settings["mode"] == "swa" else "n_upd"
    return {"mode": settings["mode"], "decay": float(settings["decay"]), "warmup": bool(settings["warmup"]), key: int(count), "average": avg}


def block_count(block: dict) -> int:
    return int(block["models_num" if block["mode"] == "swa" else "n_upd"])


def settings_mismatches(block: Optional[dict], settings: Optional[dict]) -> list:
    """[(name, checkpoint value, trainer value)] over mode / decay / warm-up when both sides average."""
    if block is None or settings is None:
        return []
    return [("weight_average." + k, block[k], settings[k]) for k in ("mode", "decay", "warmup") if block.get(k) != settings[k]]


def reconcile(block: Optional[dict], settings: Optional[dict], strict: bool, n_params: Optional[int] = None) -> str:
    """What a load does with the block of a checkpoint (`block`, None when the file has none) given the trainer's averaging settings
    (None when it does not average): "none" (neither side averages), "load" (copy the average and its count in place), "reinit" (the
    average becomes a copy of the loaded parameters) or "ignore" (the trainer does not average).  strict refuses what differs, naming it.
    A block of another parameter count is refused either way."""
    if block is None and settings is None:
        return "none"
    if block is not None and n_params is not None and tuple(block["average"].shape) != (int(n_params),):
        raise ValueError(f"checkpoint: the weight average has shape {tuple(block['average'].shape)}, expected ({int(n_params)},)")
    if block is None:
        if strict:
            raise ValueError(f"the checkpoint carries no weight average, the trainer averages (mode {settings['mode']!r}): weight_average: "
                             "checkpoint None, trainer set (strict=False loads the tensors and re-initialises the average from them)")
        return "reinit"
    if settings is None:
        if strict:
            raise ValueError(f"the checkpoint carries a weight average (mode {block['mode']!r}), the trainer does not average: "
                             "weight_average: checkpoint set, trainer None (strict=False ignores the block)")
        return "ignore"
    bad = settings_mismatches(block, settings)
    if bad and strict:
        raise ValueError("the checkpoint's weight average was kept under other settings: " +
                         "; ".join(f"{k}: checkpoint {a!r}, trainer {b!r}" for k, a, b in bad))
    # another mode counts other things (models vs. updates): the tensors do not continue this trainer's series
    return "reinit" if block["mode"] != settings["mode"] else "load"


class WeightAverage:
    """avg: a flat fp32 device tensor like engine.params, created as a copy of the parameters.
    mode "swa": update() is swa_step -- models_num += 1, beta = 1.0 / models_num, avg = avg * (1 - beta) + p * beta; the caller decides
    when (fit: before every validation from swa_epoch_start on).  mode "ema": update() is one exponential update with the decay series
    ema_decay(n_upd, decay, warmup), count and weights on the device, so it is valid inside a captured step; `skip_flag` (the guarded
    optimizer's skipped flag, a device scalar) makes it a no-op for a skipped optimizer step.  Every buffer is allocated here, once: a
    captured step addresses them by pointer, and loading writes INTO them."""

    def __init__(self, engine, mode: str, decay: float = 0.999, warmup: bool = True):
        import torch

        from . import _lib
        self._settings = check_settings(mode, decay, warmup)
        self.engine, self.mode, self.decay, self.warmup = engine, mode, float(decay), bool(warmup)
        self.lib = _lib.hip()
        self.avg = engine.params.clone()
        self.models_num = 1
        # "ema": the device state (include/pmgt_capi.h): int64 [0] n_upd, 32-bit words [2] skip word, [3] w_old, [4] w_new
        self.state = torch.zeros(_lib.AVG_STATE_BYTES // 8, dtype=torch.int64, device=engine.device) if mode == "ema" else None

    def settings(self) -> dict:
        return dict(self._settings)

    def key(self) -> tuple:
        """What a captured step freezes of the averaging."""
        return (self.mode, self.decay, self.warmup)

    def init_from_params(self) -> None:
        """swa_init (pmgt/utils/train.py:39-50): the average is the current parameters, models_num = 1 / n_upd = 0.  In place."""
        self.avg.copy_(self.engine.params)
        self.models_num = 1
        if self.state is not None:
            self.state.zero_()

    def update(self, skip_flag=None) -> None:
        from . import _lib
        eng = self.engine
        if self.mode == "swa":
            self.models_num += 1
            w_old, w_new = swa_weights(self.models_num)
            cfg = _lib.AvgStepC(0, 0, 0.0, None, None, float(w_old), float(w_new))
        else:
            cfg = _lib.AvgStepC(1, int(self.warmup), self.decay, self.state.data_ptr(), None if skip_flag is None else skip_flag.data_ptr(),
                                0.0, 0.0)
        _lib.check(self.lib.pmgt_weight_average_update(self.avg.data_ptr(), eng.params.data_ptr(), eng.n_params, C.byref(cfg), _lib.stream()))

    def swap(self) -> None:
        """Exchanges the contents of the average and the parameter buffer (swap_swa_params' effect, pmgt/utils/train.py:72-85)."""
        from . import _lib
        _lib.check(self.lib.pmgt_weight_swap(self.avg.data_ptr(), self.engine.params.data_ptr(), self.engine.n_params, _lib.stream()))

    def count(self) -> int:
        """models_num ("swa", a host int) or n_upd ("ema": one small device -> host read)."""
        return int(self.models_num) if self.mode == "swa" else int(self.state[0].item())

    def device_state(self) -> dict:
        """"ema": {n_upd, skipped, w_old, w_new} as the device holds them (one small read)."""
        import torch
        st = self.state.cpu()
        f, w = st.view(torch.float32), st.view(torch.int32)
        return {"n_upd": int(st[0]), "skipped": int(w[2]), "w_old": f[3].item(), "w_new": f[4].item()}

    def state_dict(self) -> dict:
        return average_block(self._settings, self.count(), self.avg.cpu())

    def load_state_dict(self, block: dict) -> None:
        """In place (copy_), as all engine state: captured steps stay valid.  The block's settings are the caller's to compare
        (reconcile); a block of the other mode is refused here."""
        import torch
        if block["mode"] != self.mode:
            raise ValueError(f"weight average of mode {block['mode']!r} cannot continue one of mode {self.mode!r}")
        if tuple(block["average"].shape) != tuple(self.avg.shape):
            raise ValueError(f"weight average has shape {tuple(block['average'].shape)}, expected {tuple(self.avg.shape)}")
        self.avg.copy_(torch.as_tensor(block["average"]).to(torch.float32))
        if self.mode == "swa":
            self.models_num = block_count(block)
        else:
            self.state.zero_()
            self.state[0] = block_count(block)
