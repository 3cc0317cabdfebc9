"""fit: the reference's driver (pmgt/base_trainer.py:283-336: pl.Trainer.fit with max_epochs, validation every epoch,
EarlyStopping(monitor, patience, mode), ModelCheckpoint(save_top_k=1, save_last=True), resume through ckpt_path) and the bookkeeping of
its two callbacks."""
from __future__ import annotations

import contextlib
import os
from typing import TYPE_CHECKING, Optional

import numpy as np
import torch

from .datasets import MODE_TRAIN
from .evaluation import batch_to_device, evaluate
from .parallel import shard_indices, world

if TYPE_CHECKING:
    from .trainer import Trainer


def monitor_of(early_criterion: str):
    """(monitor, mode) as init_run derives them (pmgt/base_trainer.py:283-286)."""
    if early_criterion == "loss":
        return "loss/val", "min"
    return f"val/{early_criterion}", "max"


def _improves(mode: str, value: float, best: Optional[float]) -> bool:
    """Strictly better (torch.lt / torch.gt in both Lightning callbacks): a tie is not an improvement."""
    if mode not in ("min", "max"):
        raise ValueError(f"mode={mode!r}: expected 'min' or 'max'")
    return best is None or (value < best if mode == "min" else value > best)


class EarlyStopping:
    """Lightning's EarlyStopping(monitor, patience, mode) with its defaults (min_delta 0, checked after every validation): `update`
    returns True once `patience` validations in a row brought no improvement."""

    def __init__(self, monitor: str, patience: int, mode: str):
        self.monitor, self.patience, self.mode = monitor, int(patience), mode
        self.wait_count, self.best_score, self.stopped_epoch = 0, None, 0

    @property
    def state_key(self) -> str:
        return f"EarlyStopping{{'monitor': '{self.monitor}', 'mode': '{self.mode}'}}"

    def update(self, value: float, epoch: int = 0) -> bool:
        if _improves(self.mode, float(value), self.best_score):
            self.best_score, self.wait_count = float(value), 0
            return False
        self.wait_count += 1
        if self.wait_count >= self.patience:
            self.stopped_epoch = int(epoch)
            return True
        return False

    def state_dict(self) -> dict:
        return {"wait_count": self.wait_count, "stopped_epoch": self.stopped_epoch, "patience": self.patience,
                "best_score": None if self.best_score is None else torch.tensor(self.best_score, dtype=torch.float64)}

    def load_state_dict(self, sd: dict) -> None:
        self.wait_count, self.stopped_epoch = int(sd["wait_count"]), int(sd.get("stopped_epoch", 0))
        self.best_score = None if sd.get("best_score") is None else float(sd["best_score"])


class BestCheckpoint:
    """The bookkeeping of ModelCheckpoint(monitor, mode, save_top_k=1, save_last=True) with the reference's file-name pattern
    `epoch={epoch:02d}-{loss|auc}={value:.4f}.ckpt` (pmgt/base_trainer.py:291-298).  No file is touched here: `update` says which
    path to write and which to remove."""

    def __init__(self, dirpath: str, monitor: str, mode: str):
        self.dirpath, self.monitor, self.mode = str(dirpath), monitor, mode
        self.best_model_path, self.best_model_score = "", None
        self.last_model_path = ""

    @property
    def state_key(self) -> str:
        return (f"ModelCheckpoint{{'monitor': '{self.monitor}', 'mode': '{self.mode}', 'every_n_train_steps': 0, 'every_n_epochs': 1, "
                "'train_time_interval': None, 'save_on_train_epoch_end': True}")

    def filename(self, epoch: int, value: float) -> str:
        # the criterion's name: "loss" of loss/val, "auc" of val/auc (the reference's own split('/')[-1] would call the first one "val")
        short = next(p for p in self.monitor.split("/") if p != "val")
        return f"epoch={int(epoch):02d}-{short}={float(value):.4f}.ckpt"

    def update(self, epoch: int, value: float):
        """(path to write, path to remove) when `value` is the best so far, (None, None) otherwise."""
        if not _improves(self.mode, float(value), self.best_model_score):
            return None, None
        old = self.best_model_path or None
        self.best_model_path, self.best_model_score = os.path.join(self.dirpath, self.filename(epoch, value)), float(value)
        return self.best_model_path, (old if old != self.best_model_path else None)

    def state_dict(self) -> dict:
        score = None if self.best_model_score is None else torch.tensor(self.best_model_score, dtype=torch.float64)
        return {"monitor": self.monitor, "best_model_score": score, "best_model_path": self.best_model_path, "current_score": score,
                "dirpath": self.dirpath, "last_model_path": self.last_model_path}

    def load_state_dict(self, sd: dict) -> None:
        self.best_model_path = str(sd.get("best_model_path") or "")
        self.best_model_score = None if sd.get("best_model_score") is None else float(sd["best_model_score"])
        self.last_model_path = str(sd.get("last_model_path") or "")


def epoch_order(n: int, seed: int, epoch: int, rank: int = 0, world_size: int = 1) -> np.ndarray:
    """Positions into the training ids this rank visits in epoch `epoch`: its strided shard of ONE permutation of 0 .. n - 1 seeded by
    (seed, epoch) (parallel.shard_indices: DistributedSampler semantics).  A pure function of its arguments: every rank computes the
    same permutation, and a resumed run the same one again."""
    return shard_indices(int(n), int(rank), int(world_size), seed=int(seed), epoch=int(epoch), shuffle=True)


def fit(trainer: Trainer, model_or_engine, sampler, train_ids: np.ndarray, valid_ids: np.ndarray, batch_size: int, max_epochs: int,
        early_criterion: str = "loss", patience: int = 10, ckpt_dir: str = ".", resume_from: Optional[str] = None,
        save_every_n_steps: int = 0, seed: int = 0, graphs: bool = False, threads: int = 8, valid_batch_size: int = 256, log=None,
        nonfinite="keep", step_log="keep", max_skipped_in_a_row="keep", eval_metrics: str = "host", swa_epoch_start=None) -> dict:
    """pl.Trainer.fit as the reference's init_run configures it, restated: `max_epochs` epochs; epoch e trains on this rank's shard of
    a permutation of `train_ids` seeded by (seed, e) -- the len // batch_size full batches through run_live, a remainder as one eager
    train_step of its true size (DataLoader drop_last=False), an unfinished accumulation window stepped at the end of the epoch as
    Lightning does; validation after every epoch (evaluate; over all ranks under a process group); monitor loss/val (min) or
    val/<criterion> (max); stop after `patience` validations without improvement; `last.ckpt` after every epoch and every
    `save_every_n_steps` optimizer steps (> 0), the single best checkpoint under the reference's name pattern with its predecessor
    removed.  resume_from: a path, or "last" (= ckpt_dir/last.ckpt): restores weights, optimizer, counters, RNG, the early-stopping and
    best-checkpoint bookkeeping and the position inside the epoch, and continues as the uninterrupted run would have.
    log: optional callable, log({"event": "train", epoch, global_step, batches_done, loss}) after every run of training steps between two
    checkpoint opportunities and log({"event": "valid", epoch, global_step, <metrics>}) after every validation.
    nonfinite / step_log / max_skipped_in_a_row: passed through to the trainer (Trainer.__init__ states them; "keep" leaves the trainer's
    own).  With either of the first two set, an epoch's history entry also carries `skipped_steps` (optimizer steps of the epoch skipped for
    a non-finite gradient norm) and, with a step log, `loss/train`: the mean loss over the epoch's applied steps that are still in the ring
    (NaN when there is none; a resume empties the ring).  Trainer.check_nonfinite runs at the end of every run of training steps, at the
    end of an epoch and before every checkpoint write: a run that trips it stops with NonFiniteGradientsError BEFORE that write, so the
    previous last.ckpt stays.
    eval_metrics: "host" (default) or "device", passed to evaluate(metrics=...) for the validation after every epoch.  Not part of the training
    state: a checkpoint written under one setting resumes under the other.
    swa_epoch_start: the reference's StochasticWeightAveraging callback (pmgt/callbacks.py:44-381), restated: an int >= 1 or a float in
    [0, 1] (then int(max_epochs * f)); at the start of the 0-based training epoch max(start - 1, 0) the average becomes a copy of the
    parameters (swa_init), and from then on every validation is preceded by swa_step (models_num += 1, avg = avg * (1 - 1 / models_num) +
    p / models_num) and a swap-in of the average, and followed by the swap back: the monitored metric, early stopping and the best
    checkpoint follow the AVERAGED model, the files hold the raw weights plus the average (Trainer.state_dict's weight_average block, and
    `average_model` under the callback's name).  Needs a trainer whose average is in "swa" mode; one is attached when the trainer keeps
    none.  The callback's SWALR scheduler swap and its BatchNorm branches are not restated: the rate stays the trainer's schedule.
    A trainer that averages in "ema" mode validates on its average from the first epoch on (the same swap around evaluate, no swa_step).
    Every rank's parameters are identical after the all-reduced step, so every rank's average is too: no collective is added.
    Returns {best_model_path, best_model_score, epochs_run, stopped_early, history: per-epoch metrics}."""
    from . import io as pio
    eng = trainer.engine
    if getattr(model_or_engine, "engine", model_or_engine) is not eng:
        raise ValueError("fit: the trainer drives another engine than the one passed")
    if eval_metrics not in ("host", "device"):
        raise ValueError(f"eval_metrics={eval_metrics!r}: expected 'host' or 'device'")
    passed = {k: v for k, v in (("nonfinite", nonfinite), ("step_log", step_log), ("max_skipped_in_a_row", max_skipped_in_a_row)) if v != "keep"}
    trainer.set_guard(**passed)                           # (run_live re-captures: nonfinite and step_log are part of _hyper_key())
    swa_start, swa_key = None, "StochasticWeightAveraging"
    if swa_epoch_start is not None:
        from .averaging import WeightAverage, swa_start_epoch
        swa_start = swa_start_epoch(swa_epoch_start, max_epochs)          # the reference's check and message
        if trainer.weight_average is None:
            trainer.weight_average = WeightAverage(eng, "swa")            # before a resume reads the file, and before any capture
        elif trainer.weight_average.mode != "swa":
            raise ValueError(f"fit(swa_epoch_start=...): the trainer averages in {trainer.weight_average.mode!r} mode; the epoch-wise "
                             "running mean needs a trainer whose weight_average is in 'swa' mode")
        # Lightning's state key of the callback; on_fit_start has turned a float into the epoch number by then
        start = int(int(max_epochs) * swa_epoch_start) if isinstance(swa_epoch_start, float) else int(swa_epoch_start)
        swa_key = f"StochasticWeightAveraging{{'swa_epoch_start': {start!r}, 'annealing_strategy': 'cos'}}"
    rank, ws = world() if trainer.world_size > 1 else (0, 1)
    monitor, mode = monitor_of(early_criterion)
    stopper, best = EarlyStopping(monitor, patience, mode), BestCheckpoint(ckpt_dir, monitor, mode)
    last_path = os.path.join(ckpt_dir, "last.ckpt")
    best.last_model_path = last_path
    if rank == 0:
        os.makedirs(ckpt_dir, exist_ok=True)
    train_ids, valid_ids = np.asarray(train_ids), np.asarray(valid_ids)
    run = {"seed": int(seed), "batch_size": int(batch_size), "n_train": int(len(train_ids)), "world_size": int(ws)}
    epoch, done, history, stopped = 0, 0, [], False
    at_epoch_start = None                                    # step counters at the start of the current epoch (guarded trainers)
    if resume_from is not None:
        ck = pio.load_training_checkpoint(model_or_engine, trainer, last_path if resume_from == "last" else resume_from)
        st = (ck.get("pmgt_amd") or {}).get("fit")
        if st is None:
            raise ValueError("fit(resume_from=...): the checkpoint was not written by fit (no epoch position in it)")
        for k, v in run.items():
            if st[k] != v:
                raise ValueError(f"fit(resume_from=...): the checkpoint was written with {k} = {st[k]!r}, this call has {v!r}: the epoch "
                                 "order and the sampler streams would not continue it")
        epoch, done, history, stopped = int(st["epoch"]), int(st["batches_done"]), [dict(h) for h in st["history"]], bool(st["stopped_early"])
        stopper.load_state_dict(pio._callback(ck["callbacks"], "EarlyStopping"))
        best.load_state_dict(pio._callback(ck["callbacks"], "ModelCheckpoint"))
        best.dirpath, best.last_model_path = str(ckpt_dir), last_path
        at_epoch_start = st.get("counters_at_epoch_start")

    def save(path, top_epoch):
        trainer.check_nonfinite()                            # on every rank, before rank 0 writes anything
        st = dict(run, epoch=epoch, batches_done=done, history=history, stopped_early=stopped, counters_at_epoch_start=at_epoch_start)
        pio.save_training_checkpoint(model_or_engine, trainer, path, epoch=top_epoch, fit=st, swa_key=swa_key,
                                     callbacks={stopper.state_key: stopper.state_dict(), best.state_key: best.state_dict()})

    def say(event, **kw):
        if log is not None:
            log(dict(event=event, epoch=epoch, global_step=trainer._opt_steps, **kw))

    stream_seed = int(seed) + rank                       # ranks see different targets: their sampler streams differ too
    while epoch < max_epochs and not stopped:
        order = train_ids[epoch_order(len(train_ids), seed, epoch, rank, ws)]
        if swa_start is not None and epoch == swa_start and done == 0:
            trainer.weight_average.init_from_params()        # swa_init, on_train_epoch_start (a resume inside this epoch finds it in the file)
        if trainer._guard() is not None and (at_epoch_start is None or done == 0):
            at_epoch_start = eng.step_counters()
        n_full = len(order) // batch_size
        chunk = save_every_n_steps * trainer.accum if save_every_n_steps > 0 else max(n_full, 1)
        while done < n_full:
            k = min(chunk - done % chunk, n_full - done)
            ids = order[done * batch_size: (done + k) * batch_size]
            # run_live wraps its slice position at len(node_ids) - batch_size: one id more than the k batches keeps every slice exact
            trainer.run_live(sampler, np.concatenate([ids, ids[:1]]), batch_size, k, threads=threads, graphs=graphs,
                             first_step=trainer.pipeline_step, base_seed=stream_seed)
            done += k
            if save_every_n_steps > 0 and trainer._micro == 0 and done < n_full:
                save(last_path, epoch)
            say("train", batches_done=done, loss=float(trainer.last_loss))
        if len(order) > n_full * batch_size and done == n_full:
            rest = sampler.batch(order[n_full * batch_size:], MODE_TRAIN, threads=threads, base_seed=stream_seed,
                                 counter=trainer.pipeline_step * batch_size)
            trainer.train_step(batch_to_device(rest, eng.device))
            trainer.pipeline_step += 1
            done += 1
            say("train", batches_done=done, loss=float(trainer.last_loss))
        trainer.flush_accumulation()
        train_metrics = {}
        counters = trainer.check_nonfinite()
        if counters is not None:
            train_metrics["skipped_steps"] = counters["skipped"] - at_epoch_start["skipped"]
            if trainer.step_log:
                mine = [r["loss"] for r in eng.step_log() if r["attempt"] >= at_epoch_start["attempts"] and not r["skipped"]]
                train_metrics["loss/train"] = float(np.mean(mine)) if mine else float("nan")
        wa = trainer.weight_average
        averaged = wa is not None and (wa.mode == "ema" or (swa_start is not None and epoch >= swa_start))
        if averaged and wa.mode == "swa":
            wa.update()                                      # swa_step, on_validation_start
        with (trainer.averaged_weights() if averaged else contextlib.nullcontext()):      # swap_swa_params around the validation
            metrics = evaluate(eng, sampler, valid_ids, batch_size=valid_batch_size, threads=threads, seed=seed, distributed=ws > 1,
                               metrics=eval_metrics)
        history.append(dict(epoch=epoch, **metrics, **train_metrics))
        top_epoch = epoch
        new_best, old_best = best.update(epoch, metrics[monitor])
        stopped = stopper.update(metrics[monitor], epoch)
        epoch, done = epoch + 1, 0
        if new_best is not None:
            save(new_best, top_epoch)
            if old_best is not None and rank == 0 and os.path.exists(old_best):
                os.unlink(old_best)
        save(last_path, top_epoch)
        say("valid", **metrics)
    return {"best_model_path": best.best_model_path, "best_model_score": best.best_model_score, "epochs_run": epoch,
            "stopped_early": stopped, "history": history}
