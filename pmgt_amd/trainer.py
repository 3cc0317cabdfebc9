"""Trainer step of the PMGT pre-training hot path (reference: `PMGTTrainerModel.training_step`,
pmgt/pmgt/trainer.py:156-160, driven by PL's loop with `gradient_clip_val`, `DenseSparseAdamW` from
`get_optimizer`, and DDP when gpus > 1 — pmgt/base_trainer.py:35-68,309-322).

Data parallelism: one process per GPU, every rank holds a full replica (graph on the
host, feature tables + weights on the device); the ONLY exchange is one all-reduce(AVG) of the flat
fp32 gradient buffer per optimizer step over RCCL/xGMI (12 MB at L4/d256: far below one link's
bandwidth-delay product, so a single un-bucketed collective is the right shape); the clip uses the
post-reduce global norm, identical on all ranks.  Each rank takes indices rank::world of one seeded
permutation (DistributedSampler semantics).
"""
from __future__ import annotations

import contextlib
import gc
import weakref
from typing import Optional

import numpy as np
import torch

from .parallel import BucketedAllReduce, allreduce_mean_, broadcast_

_KEEP = object()      # Trainer.set_guard: a setting that is not passed


class NonFiniteGradientsError(RuntimeError):
    """Too many optimizer steps in a row were skipped for a non-finite gradient norm (Trainer.check_nonfinite): the run is not
    recovering by itself.  `counters` = Engine.step_counters() at the time."""

    def __init__(self, message, counters=None):
        super().__init__(message)
        self.counters = dict(counters or {})


class Trainer:
    def __init__(self, engine, lr: float = 1e-3, weight_decay: float = 1e-2, betas=(0.9, 0.999), eps: float = 1e-8,
                 max_grad_norm: Optional[float] = None, world_size: int = 1, accumulate_grad_batches: int = 1,
                 random_node_ratio: float = 0.02, mask_node_ratio: float = 0.16, overlap_allreduce: bool = True,
                 buckets: str = "two", check_carrier_every: int = 200, force_exchange: bool = False,
                 scheduler_type: Optional[str] = None, num_warmup_steps: Optional[int] = None,
                 num_training_steps: Optional[int] = None, nonfinite: Optional[str] = None, step_log: int = 0,
                 max_skipped_in_a_row: int = 25, weight_average=None):
        """scheduler_type (one of the reference's --scheduler-type choices; None = constant `lr`, the step as it always was) with
        num_warmup_steps / num_training_steps: every optimizer step uses lr * lambda(k), k = the optimizer steps completed before
        it, evaluated ON THE DEVICE by the fused step (pmgt_amd.schedule states the multipliers).  It advances once per optimizer
        step, so gradient accumulation and data parallelism (every rank's counter is equal) need nothing more, and a captured
        step / run_live(graphs=True) follows it with no re-capture.  The schedule's position is `engine.opt_step`, the same
        device counter as Adam's bias corrections: setting that counter, as a resume does (load_state_dict), moves both together.

        nonfinite="skip": what the GradScaler of the reference's --mp-enabled run does (pmgt/base_trainer.py:312) -- an optimizer step
        whose gradients hold an Inf or a NaN (global norm not finite; that includes a sum of squares past fp32, for which
        clip_grad_norm_ reports Inf too) is skipped, decided ON THE DEVICE inside the fused step, so it holds in a captured step and
        under run_live(graphs=True) with no host sync: parameters, moments and opt_step stay as they were, so bias corrections and
        the schedule count applied steps only.  With accumulation the window's gradients are dropped: the next micro-batch overwrites
        the buffer.  Under data parallelism the decision is taken after the all-reduce, on gradients that are identical on every
        rank: every rank decides alike and no extra collective is needed.  step_log=R keeps the last R optimizer steps (loss of the
        step's last micro-batch, pre-clip norm, clip coefficient, rate, skipped flag) in a device ring, Engine.step_log(); alone it
        logs without guarding.  Both are frozen into a captured step and recorded in checkpoints like the other hyper-parameters.
        None / 0 (default): the step through the entries it always took.  max_skipped_in_a_row: check_nonfinite() raises
        NonFiniteGradientsError at that many consecutive skips (25 is a policy default, not a measurement); it runs only where the
        host waits for the GPU anyway (end of run_live, epoch end and checkpoint writes of fit, state_dict()), never per step.

        weight_average: None (default: the step through the entries it always took), a pmgt_amd.averaging.WeightAverage over this engine,
        or a dict of its arguments (mode="swa" | "ema", decay=0.999, warmup=True).  The average starts as a copy of the parameters as they
        are NOW (load them first, or call weight_average.init_from_params()).  "ema": every optimizer step is followed by one exponential
        update of the average ON THE DEVICE (count and decay there too), so a captured step / run_live(graphs=True) simply records the
        two extra launches, and with nonfinite="skip" a skipped optimizer step is not averaged in.  "swa": the step does nothing extra; the
        running mean is updated by whoever decides when (fit(swa_epoch_start=...): before every validation).  averaged_weights() puts the
        average into the parameter buffer for forward work.  The settings are frozen into a captured step and the average travels in
        checkpoints."""
        self.engine = engine
        self.weight_average = None
        self._averaged = False        # inside averaged_weights(): the parameter buffer holds the average
        if weight_average is not None:
            from .averaging import WeightAverage
            wa = WeightAverage(engine, **weight_average) if isinstance(weight_average, dict) else weight_average
            if not isinstance(wa, WeightAverage):
                raise ValueError(f"weight_average={weight_average!r}: expected None, a WeightAverage or a dict of its arguments")
            if wa.engine is not engine:
                raise ValueError("weight_average: the WeightAverage was built over another engine than the trainer's")
            self.weight_average = wa
        self.set_guard(nonfinite=nonfinite, step_log=step_log, max_skipped_in_a_row=max_skipped_in_a_row)
        self.scheduler_type, self.num_warmup_steps, self.num_training_steps = scheduler_type, num_warmup_steps, num_training_steps
        if scheduler_type is not None:
            from .schedule import lr_lambda
            lr_lambda(scheduler_type, num_warmup_steps, num_training_steps, lr)       # refuses what the device step would refuse
        # force_exchange: run the data-parallel exchange (bucketed all-reduce from the engine's callback, wait in front of the optimizer)
        # even with ONE rank -- the N > 1 code path unchanged on a single-rank process group, so that RCCL executes it on a one-GPU box
        self.force_exchange = bool(force_exchange)
        self.lr, self.weight_decay, self.betas, self.eps = lr, weight_decay, betas, eps
        self.max_grad_norm = max_grad_norm
        self.world_size = world_size
        self.accum = max(1, accumulate_grad_batches)
        self.random_node_ratio, self.mask_node_ratio = random_node_ratio, mask_node_ratio
        self.last_loss = None
        self.last_outputs = None      # the output set of the last training_step
        self._micro = 0
        self._capturing = False       # inside capture_step's stream capture: the step writes an output set of its own
        # run_live: pinned host + device slot buffers by shape, and (slot buffers, shape, hyper-parameters) -> captured step; both live
        # as long as the trainer
        self._live_slots, self._live_replays = {}, {}
        # every N optimizer steps re-check that the LayerNorm parameters still allow x^ = (y - beta) / gamma from the bf16 output
        # (Engine.check_layernorm_carrier: one small device -> host read per LayerNorm; 0 = only when parameters are loaded or a
        # step is captured)
        self.check_carrier_every = int(check_carrier_every)
        self._opt_steps = 0
        # global index of the next step of the live input pipeline (run_live / fit): the sampler streams of step g start at counter
        # g * batch_size, so a call that starts where the last one ended draws no stream twice.  Part of state_dict().
        self.pipeline_step = 0
        # world_size > 1: per-bucket all-reduce started from the engine's gradient-ready hook while the backward pass of
        # the earlier layers is still running (overlap_allreduce=False: ONE blocking all-reduce after the backward pass)
        self._exchange = None
        # buckets: "layer" = one collective per engine bucket (NFR head, every layer, embeddings); "two" = NFR head + encoder
        # layers as one collective (issued when layer 0's gradients are final), embeddings as the second; "one" = the whole buffer
        # after the backward pass (engine option one_bucket).  Default "two" = bench.py's default (one policy for the library and the measurement);
        # PROVISIONAL: chosen on one-rank RCCL runs (profiles/r05/rccl_single_rank_exchange.txt), where transport is free -- no multi-GPU A/B exists
        if buckets not in ("layer", "two", "one"):
            raise ValueError(f"buckets={buckets!r}: expected 'layer', 'two' or 'one'")
        self.buckets = buckets
        if self._exchanging and overlap_allreduce:
            bounds = ()
            if buckets == "two" and engine.config.num_hidden_layers > 0:
                bounds = (engine.entry("bert.encoder.layer.0.attention.self.query.weight")["offset"],)
            engine.set_option("one_bucket", buckets == "one")
            self._exchange = BucketedAllReduce(engine.grads, boundaries=bounds)
            engine.set_grad_ready_hook(self._exchange.bucket_ready)

    def set_guard(self, nonfinite=_KEEP, step_log=_KEEP, max_skipped_in_a_row=_KEEP):
        """Checks and assigns the guard settings that are passed (__init__ states them); the others stay.  In the check and its message a
        setting that is not passed stands at the constructor's default, as in a constructor call with the passed ones alone."""
        if nonfinite is not _KEEP and nonfinite not in (None, "skip"):
            raise ValueError(f"nonfinite={nonfinite!r}: expected None or 'skip'")
        rows, most = 0 if step_log is _KEEP else step_log, 25 if max_skipped_in_a_row is _KEEP else max_skipped_in_a_row
        if int(rows) < 0 or int(most) < 1:
            raise ValueError(f"step_log={rows!r} must be >= 0 and max_skipped_in_a_row={most!r} >= 1")
        if nonfinite is not _KEEP:
            self.nonfinite = nonfinite
        if step_log is not _KEEP:
            self.step_log = int(step_log)
        if max_skipped_in_a_row is not _KEEP:
            self.max_skipped_in_a_row = int(max_skipped_in_a_row)

    _exchanging = property(lambda self: self.world_size > 1 or self.force_exchange)      # the data-parallel exchange precedes the optimizer step
    _capturable = property(lambda self: self.world_size == 1 and self.accum == 1 and not self.force_exchange)      # what capture_step covers

    def broadcast_parameters(self, src: int = 0):
        """DDP constructor semantics: every replica starts from rank `src`'s parameters."""
        if self._exchanging:
            broadcast_(self.engine.params, src=src, force=self.force_exchange)

    def training_step(self, batch, batch_idx: int = 0) -> torch.Tensor:
        """loss = net(*batch)[0] with gradients left in engine.grads (pmgt/pmgt/trainer.py:156-160).  The returned device
        scalar lives in the engine's output ring (valid for the next Engine.OUTPUT_RING - 1 steps; clone it to keep it)."""
        self._not_averaged("training_step")
        if self._exchange is not None:      # gradients are exchanged once per optimizer step: on the last micro-batch
            self._exchange.enabled = self._exchanging and self._micro == self.accum - 1
        out = self.engine.pretrain_step(batch, training=True, backward=True, accumulate=self._micro > 0,
                                        random_node_ratio=self.random_node_ratio, mask_node_ratio=self.mask_node_ratio,
                                        want_hidden=False, private_outputs=self._capturing)
        self.last_loss = out["loss"]
        self.last_outputs = out
        return out["loss"]

    def optimizer_step(self):
        self._not_averaged("optimizer_step")
        eng = self.engine
        if self._exchanging:
            done = self._exchange.wait() if self._exchange is not None else 0
            if done == 0:
                allreduce_mean_(eng.grads, force=self.force_exchange)
            elif done != eng.n_params:
                raise RuntimeError(f"gradient exchange covered {done} of {eng.n_params} elements")
        if self.accum > 1:
            eng.grads.div_(self.accum)
        eng.optimizer_step(lr=self.lr, weight_decay=self.weight_decay, betas=self.betas, eps=self.eps,
                           max_grad_norm=self.max_grad_norm, schedule=self._schedule(), guard=self._guard())
        wa = self.weight_average
        if wa is not None and wa.mode == "ema":
            # behind the optimizer on the same stream; the guard's skipped flag (scal[5]) keeps a skipped step out of the average
            wa.update(skip_flag=eng.was_skipped() if self.nonfinite == "skip" else None)
        self._opt_steps += 1
        if self.check_carrier_every and self._opt_steps % self.check_carrier_every == 0 and not self._capturing:
            self._check_carrier()

    def _check_carrier(self):
        """The periodic LayerNorm-carrier guard of an EAGER step.  When the guard has to switch the engine to stored LayerNorm inputs while
        captured steps are alive, the ones this trainer owns (run_live(graphs=True)) are dropped first -- run_live re-captures them on its next
        call, exactly as its own periodic check does -- so a user who mixes run_live(graphs=True) with later eager train_step calls does not
        meet an error at the flip.  Replay handles the CALLER holds (capture_step) cannot be dropped from here: that case keeps the engine's
        error, which names the remedy."""
        if self.engine.carrier_needs_stored_inputs():      # (the engine's own condition for switching: its check only reads otherwise)
            self._release_captured_steps()
            self.engine.check_layernorm_carrier()

    def _release_captured_steps(self):
        """drop_captured_steps() and a collection, so that the graphs are destroyed and counted out of the engine before an option changes."""
        if self._live_replays:
            self.drop_captured_steps()
            gc.collect()

    def train_step(self, batch) -> torch.Tensor:
        """One micro-batch; steps the optimizer every `accumulate_grad_batches` calls."""
        self._not_averaged("train_step")
        loss = self.training_step(batch)
        self._micro += 1
        if self._micro == self.accum:
            self.optimizer_step()
            self._micro = 0
        return loss

    def flush_accumulation(self):
        """Steps the optimizer on an accumulation window that the end of an epoch cut short (Lightning steps on the last batch of an epoch
        whatever the window holds; the gradients keep their 1 / accumulate_grad_batches scale).  Nothing to do at a window boundary."""
        if self._micro:
            self.optimizer_step()
            self._micro = 0

    # ---- the averaged weights in the parameter buffer, for forward work ------------------------------------------------------
    def _not_averaged(self, what: str):
        if self._averaged:
            raise RuntimeError(f"Trainer.{what}() inside Trainer.averaged_weights(): the parameter buffer holds the AVERAGED weights there; "
                               "only forward work (evaluate, encode, export_embeddings) belongs inside that context")

    @contextlib.contextmanager
    def averaged_weights(self):
        """Context manager: exchanges the CONTENTS of the parameter buffer and the average on entry and back on exit (also when the body
        raises), so evaluate / encode / export_embeddings inside see the averaged model through the same pointers -- captured steps taken
        before stay valid afterwards.  Training entries raise inside; entering it twice raises.  No LayerNorm-carrier re-check runs:
        the carrier only matters to a backward pass, and none belongs here."""
        wa = self.weight_average
        if wa is None:
            raise RuntimeError("Trainer.averaged_weights(): this trainer keeps no weight average (Trainer(weight_average=...))")
        if self._averaged:
            raise RuntimeError("Trainer.averaged_weights() entered twice: the parameter buffer already holds the averaged weights")
        if self._micro != 0:
            raise RuntimeError(f"Trainer.averaged_weights(): {self._micro} of {self.accum} micro-batches of the current accumulation "
                               "window have run; swap at an optimizer-step boundary")
        wa.swap()
        self._averaged = True
        try:
            yield wa
        finally:
            wa.swap()
            self._averaged = False

    # ---- the whole step as ONE hipGraph ---------------------------------------------------------------------------
    def capture_step(self, batch, warmup: int = 2, capture_error_mode: str = "global"):
        """Captures train_step(batch) (mask -> forward -> losses -> backward -> clip + AdamW) into a hipGraph and
        returns `replay()`: the library never syncs or allocates and keeps every data-dependent count (masked rows,
        dropout step, AdamW step, and with it the scheduled learning rate) on the device, so the captured launches stay valid step
        after step.  New batches
        are fed by copying into the tensors of `batch` (static input buffers), as with any captured graph.
        `warmup` eager steps run first (one-time kernel attribute calls are not capturable).  Single-GPU step only:
        the gradient all-reduce is not captured."""
        assert self._capturable, "capture covers the single-GPU, non-accumulating step"
        self._not_averaged("capture_step")
        dev = self.engine.device
        # replays never run the Python-side guard: decide "x^ from the LayerNorm output or from stored inputs" once, on the
        # parameters as they are now, before the kernels are frozen into the graph
        self.engine.check_layernorm_carrier()
        # Adam moments exist before the capture: their zero-fill must not become a node of the graph (it would reset them on every replay)
        self.engine.ensure_optimizer_state()
        if self._guard() is not None:
            self.engine.ensure_step_log(self.step_log)       # the log ring too
        st = torch.cuda.Stream(device=dev)
        st.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(st):
            for _ in range(warmup):
                self.train_step(batch)
            st.synchronize()
            graph = torch.cuda.CUDAGraph()
            self._capturing = True        # the graph gets an output set of its own: replays keep writing it, eager steps never do
            try:
                with torch.cuda.graph(graph, stream=st, capture_error_mode=capture_error_mode):
                    loss = self.train_step(batch)
                    outputs = self.last_outputs
            finally:
                self._capturing = False
        torch.cuda.current_stream(dev).wait_stream(st)

        def replay():
            graph.replay()
            self.last_loss = loss
            return loss
        eng = self.engine
        eng._live_graphs += 1      # Engine.set_option refuses changes while a captured step lives
        weakref.finalize(graph, lambda: setattr(eng, "_live_graphs", eng._live_graphs - 1))
        replay.graph = graph
        replay.outputs = outputs          # loss / logits / nfr_count the replays write (kept alive with the graph)
        # everything the captured launches address by raw pointer lives as long as the replay handle: the engine's workspace (a later,
        # larger call makes the engine allocate a NEW one and drop its reference to this one), the static input tensors, the moments
        replay.keep = (eng._ws, batch, eng.exp_avg, eng.exp_avg_sq, eng.params, eng.grads)
        if self.weight_average is not None:      # (allocated with the WeightAverage, i.e. before this capture)
            replay.keep += (self.weight_average.avg, self.weight_average.state)
        return replay

    def _schedule(self):
        """(type, W, T) of the learning-rate schedule, or None"""
        if self.scheduler_type is None:
            return None
        return (self.scheduler_type, int(self.num_warmup_steps or 0), int(self.num_training_steps or 0))

    def _guard(self):
        """The guard argument of Engine.optimizer_step, or None when neither nonfinite nor step_log is set (the unguarded entries).  The
        loss it logs is the loss scalar of the step's last micro-batch: in a capture that is the capture's private output."""
        if self.nonfinite is None and not self.step_log:
            return None
        return dict(skip_nonfinite=self.nonfinite == "skip", log_rows=self.step_log, loss=self.last_loss)

    def check_nonfinite(self, counters: Optional[dict] = None) -> Optional[dict]:
        """Reads the step counters (one small read; pass `counters` when they were just read) and raises NonFiniteGradientsError when
        max_skipped_in_a_row or more optimizer steps in a row were skipped.  Returns the counters (None without a guard).  Under data
        parallelism every rank holds the same counters, so every rank raises alike."""
        if self._guard() is None:
            return None
        c = counters if counters is not None else self.engine.step_counters()
        if self.nonfinite == "skip" and c["skipped_in_a_row"] >= self.max_skipped_in_a_row:
            log = self.engine.step_log()
            norm = f"{log[-1]['grad_norm']!r} (attempt {log[-1]['attempt']})" if log else "not logged (step_log=0)"
            raise NonFiniteGradientsError(
                f"the last {c['skipped_in_a_row']} optimizer steps in a row were skipped for a non-finite gradient norm "
                f"(max_skipped_in_a_row={self.max_skipped_in_a_row}; {c['skipped']} of {c['attempts']} steps skipped in total; last logged "
                f"pre-clip norm: {norm}); parameters and optimizer state are those of the last applied step", c)
        return c

    def _hyper_key(self):
        """What a captured step froze into kernel arguments: a replay is only valid for the same values.  Of a learning-rate schedule
        that is its descriptor (type, W, T) and the base lr; the current rate is computed on the device and is not part of the key."""
        return tuple(self.hyper_parameters().values())

    def _capture_key(self):
        """_hyper_key() plus the averaging settings (mode, decay, warm-up) when the trainer averages: what run_live keys a captured step on."""
        if self.weight_average is None:
            return self._hyper_key()
        return self._hyper_key() + (("weight_average",) + self.weight_average.key(),)

    def drop_captured_steps(self):
        """Forgets every step run_live(graphs=True) captured (call after changing lr / weight decay / clip / ratios / engine options by
        hand; run_live itself re-captures when the hyper-parameters it was captured with no longer match).  Waits for the GPU first: a
        graph must not be destroyed while a replay of it is still executing."""
        if self._live_replays:
            torch.cuda.synchronize(self.engine.device)
            self._live_replays.clear()

    # ---- full training state: what a resume needs beyond the weights ---------------------------------------------------------
    def hyper_parameters(self) -> dict:
        """_hyper_key() by name: what decides the curve besides the data (the schedule as its descriptor (type, W, T) or None)."""
        return {"lr": float(self.lr), "weight_decay": float(self.weight_decay), "betas": tuple(float(b) for b in self.betas),
                "eps": float(self.eps), "max_grad_norm": None if self.max_grad_norm is None else float(self.max_grad_norm),
                "random_node_ratio": float(self.random_node_ratio), "mask_node_ratio": float(self.mask_node_ratio),
                "nonfinite": self.nonfinite, "step_log": int(self.step_log), "schedule": self._schedule()}

    def state_dict(self) -> dict:
        """Everything a training step mutates (Engine.training_state(): flat parameters, both Adam moments, opt_step, rng_state, path
        options) plus the trainer's own counters: the phase of the LayerNorm-carrier guard (_opt_steps), the pipeline position, the
        hyper-parameters and the accumulation factor the state was produced with.  Only at an optimizer-step boundary: between the
        micro-batches of one accumulation window the gradient buffer is part of the state, and it is not saved."""
        if self._micro != 0:
            raise RuntimeError(f"Trainer.state_dict(): {self._micro} of {self.accum} micro-batches of the current accumulation window have "
                               "run; the training state can only be saved at an optimizer-step boundary (_micro == 0)")
        est = self.engine.training_state()
        self.check_nonfinite(est["step_counters"])      # a run that no longer applies its steps is not checkpointed
        if self._averaged:
            raise RuntimeError("Trainer.state_dict() inside Trainer.averaged_weights(): the parameter buffer holds the averaged weights")
        sd = {"engine": est, "opt_steps": int(self._opt_steps), "pipeline_step": int(self.pipeline_step),
              "hyper_parameters": self.hyper_parameters(), "accumulate_grad_batches": int(self.accum)}
        if self.weight_average is not None:      # absent without averaging: the state is what it always was
            sd["weight_average"] = self.weight_average.state_dict()
        return sd

    def hyper_mismatches(self, sd: dict) -> list:
        """[(name, checkpoint value, trainer value)] over the hyper-parameters and the accumulation factor `sd` records."""
        mine = dict(self.hyper_parameters(), accumulate_grad_batches=int(self.accum))
        theirs = dict(sd.get("hyper_parameters") or {})
        if "schedule" in theirs:       # a file of this package (the reference's records no schedule) from before the guard existed: off
            theirs.setdefault("nonfinite", None)
            theirs.setdefault("step_log", 0)
        if sd.get("accumulate_grad_batches") is not None:
            theirs["accumulate_grad_batches"] = int(sd["accumulate_grad_batches"])
        norm = lambda v: tuple(norm(x) for x in v) if isinstance(v, (list, tuple)) else v
        from .averaging import settings_mismatches
        wa = self.weight_average
        return [(k, norm(theirs[k]), norm(mine[k])) for k in mine if k in theirs and norm(theirs[k]) != norm(mine[k])] + \
            settings_mismatches(sd.get("weight_average"), None if wa is None else wa.settings())

    def load_state_dict(self, sd: dict, strict: bool = True) -> None:
        """Continues from `sd` (state_dict()'s layout).  The tensors are written INTO the engine's existing buffers, so the steps
        run_live(graphs=True) captured stay valid and replay from the loaded state -- unless `sd` was produced under other
        hyper-parameters or engine path options than the live ones: those are frozen into the captured launches, so the captures are
        dropped first (run_live records them again).  strict: a hyper-parameter or accumulation factor that differs raises a
        ValueError naming both values (a silently different curve is worse); strict=False takes the checkpoint's tensors and counters
        and keeps this trainer's hyper-parameters.  A state of another parameter count, engine dtype or configuration is refused
        either way, before anything is written.
        The `weight_average` block: a state without it into a trainer that averages, or with it into a trainer that does not, raises
        under strict; strict=False re-initialises the average from the loaded parameters, respectively ignores the block.  Mode, decay
        and warm-up are compared like the other hyper-parameters.  The average and its count are written in place too."""
        from .averaging import reconcile
        eng = self.engine
        est = sd["engine"]
        eng.check_training_state(est)
        if self._averaged:
            raise RuntimeError("Trainer.load_state_dict() inside Trainer.averaged_weights()")
        wa = self.weight_average
        block = sd.get("weight_average")
        bad = self.hyper_mismatches(sd)
        options_differ = est.get("options") is not None and set(est["options"]) != set(eng.options_set())
        if bad or options_differ:
            self._release_captured_steps()
        if bad and strict:
            raise ValueError("Trainer.load_state_dict: the checkpoint was written under other hyper-parameters: " +
                             "; ".join(f"{k}: checkpoint {a!r}, trainer {b!r}" for k, a, b in bad) +
                             " (strict=False loads the tensors and counters and keeps the trainer's values)")
        averaging = reconcile(block, None if wa is None else wa.settings(), strict, eng.n_params)      # raises before anything is written
        eng.load_training_state(est)
        if averaging == "load":
            wa.load_state_dict(block)
        elif averaging == "reinit":
            wa.init_from_params()
        if est.get("rng_state") is None:
            # a checkpoint of the reference has no dropout counter: this engine's seed, at the step a run of ours would have reached
            eng.rng_state[1] = int(est["opt_step"]) * self.accum
        self._opt_steps = int(sd.get("opt_steps", est["opt_step"]))
        self.pipeline_step = int(sd.get("pipeline_step", int(est["opt_step"]) * self.accum))
        self._micro = 0

    # ---- live input pipeline: threaded C++ MCNSampling -> pinned buffers -> side-stream H2D ------------
    def run_live(self, sampler, node_ids: np.ndarray, batch_size: int, steps: int, threads: int = 8, depth: int = 3,
                 stall_timeout_s: float = 120.0, graphs: bool = False, first_step: int = 0, base_seed: int = 7):
        """Training steps fed by the live host pipeline (the reference: a DataLoader over PMGTDataset, pmgt/pmgt/trainer.py:84-105):
        ONE producer thread runs the threaded C++ sampler into a pinned host slot and issues the slot's async H2D copies on a
        side stream into that slot's PRE-ALLOCATED device buffers (no allocator call, no record_stream on the step's path); the
        launch thread orders each step behind its copies with one event and hands the slot back with a completion event.
        graphs=True: the step is captured once per slot over that slot's device buffers (train-mode batches have a fixed shape: every
        target brings max_total_samples pairs) and replayed -- ONE launch per step, so a launch thread that loses its CPU for a
        millisecond in the middle of a step's ~70 launches (a shared host) no longer shows up as GPU idle time inside the step.
        first_step: global index of this call's first step; the sampler streams of step i start at counter (first_step + i) *
        batch_size, so `first_step=trainer.pipeline_step` continues where the previous call (or a loaded checkpoint) ended instead of
        drawing its contexts and negatives again.  The default 0 restarts the streams, as every call did before the keyword existed.
        The slice of `node_ids` a step takes stays relative to the call.  `pipeline_step` is left at first_step + the steps run."""
        return live_loop(self, sampler, node_ids, batch_size, steps, threads, depth, stall_timeout_s, graphs, first_step, base_seed)


# what lived here before the split by concern stays importable from here; at the bottom: none of the three may need this module to import
from .evaluation import (EVAL_PINNED_SLOTS, encode_catalogue, evaluate, evaluate_ranking, export_embeddings, rank_users,  # noqa: E402,F401
                         ranking_metrics_host, roc_auc_score)
from .fit_loop import BestCheckpoint, EarlyStopping, epoch_order, fit, monitor_of  # noqa: E402,F401
from .pipeline import PipelineError, ProducerPipeline, live_loop  # noqa: E402,F401
