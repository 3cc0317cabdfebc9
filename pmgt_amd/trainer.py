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

import queue
import threading
import time
from typing import Optional

import numpy as np
import torch

from .datasets import MODE_EVAL, MODE_INFERENCE, MODE_TRAIN
from .parallel import BucketedAllReduce, allreduce_mean_, broadcast_, gather_predictions, world


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
        if nonfinite not in (None, "skip"):
            raise ValueError(f"nonfinite={nonfinite!r}: expected None or 'skip'")
        if int(step_log) < 0 or int(max_skipped_in_a_row) < 1:
            raise ValueError(f"step_log={step_log!r} must be >= 0 and max_skipped_in_a_row={max_skipped_in_a_row!r} >= 1")
        self.nonfinite, self.step_log, self.max_skipped_in_a_row = nonfinite, int(step_log), int(max_skipped_in_a_row)
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
        if (world_size > 1 or self.force_exchange) and overlap_allreduce:
            bounds = ()
            if buckets == "two" and engine.config.num_hidden_layers > 0:
                bounds = (engine.entry("bert.encoder.layer.0.attention.self.query.weight")["offset"],)
            engine.set_option("one_bucket", buckets == "one")
            self._exchange = BucketedAllReduce(engine.grads, boundaries=bounds)
            engine.set_grad_ready_hook(self._exchange.bucket_ready)

    def broadcast_parameters(self, src: int = 0):
        """DDP constructor semantics: every replica starts from rank `src`'s parameters."""
        if self.world_size > 1 or self.force_exchange:
            broadcast_(self.engine.params, src=src, force=self.force_exchange)

    def training_step(self, batch, batch_idx: int = 0) -> torch.Tensor:
        """loss = net(*batch)[0] with gradients left in engine.grads (pmgt/pmgt/trainer.py:156-160).  The returned device
        scalar lives in the engine's output ring (valid for the next Engine.OUTPUT_RING - 1 steps; clone it to keep it)."""
        self._not_averaged("training_step")
        if self._exchange is not None:      # gradients are exchanged once per optimizer step: on the last micro-batch
            self._exchange.enabled = (self.world_size > 1 or self.force_exchange) and self._micro == self.accum - 1
        out = self.engine.pretrain_step(batch, training=True, backward=True, accumulate=self._micro > 0,
                                        random_node_ratio=self.random_node_ratio, mask_node_ratio=self.mask_node_ratio,
                                        want_hidden=False, private_outputs=self._capturing)
        self.last_loss = out["loss"]
        self.last_outputs = out
        return out["loss"]

    def optimizer_step(self):
        self._not_averaged("optimizer_step")
        eng = self.engine
        if self.world_size > 1 or self.force_exchange:
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
        eng = self.engine
        flips = eng.layernorm_carrier_ratio() > eng.LN_CARRIER_MAX_RATIO and not eng.get_option("store_ln_input")
        if flips and eng._live_graphs > 0 and self._live_replays:
            import gc
            self.drop_captured_steps()
            gc.collect()
        eng.check_layernorm_carrier()

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

    def averaged_weights(self):
        """Context manager: exchanges the CONTENTS of the parameter buffer and the average on entry and back on exit (also when the body
        raises), so evaluate / encode / export_embeddings inside see the averaged model through the same pointers -- captured steps taken
        before stay valid afterwards.  Training entries raise inside; entering it twice raises.  No LayerNorm-carrier re-check runs:
        the carrier only matters to a backward pass, and none belongs here."""
        import contextlib

        @contextlib.contextmanager
        def ctx():
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
        return ctx()

    # ---- the whole step as ONE hipGraph ---------------------------------------------------------------------------
    def capture_step(self, batch, warmup: int = 2, capture_error_mode: str = "global"):
        """Captures train_step(batch) (mask -> forward -> losses -> backward -> clip + AdamW) into a hipGraph and
        returns `replay()`: the library never syncs or allocates and keeps every data-dependent count (masked rows,
        dropout step, AdamW step, and with it the scheduled learning rate) on the device, so the captured launches stay valid step
        after step.  New batches
        are fed by copying into the tensors of `batch` (static input buffers), as with any captured graph.
        `warmup` eager steps run first (one-time kernel attribute calls are not capturable).  Single-GPU step only:
        the gradient all-reduce is not captured."""
        assert self.world_size == 1 and self.accum == 1 and not self.force_exchange, "capture covers the single-GPU, non-accumulating step"
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
        import weakref
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
        return (float(self.lr), float(self.weight_decay), tuple(float(b) for b in self.betas), float(self.eps),
                None if self.max_grad_norm is None else float(self.max_grad_norm), float(self.random_node_ratio), float(self.mask_node_ratio),
                self.nonfinite, int(self.step_log), self._schedule())

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
    HYPER_NAMES = ("lr", "weight_decay", "betas", "eps", "max_grad_norm", "random_node_ratio", "mask_node_ratio", "nonfinite", "step_log", "schedule")

    def hyper_parameters(self) -> dict:
        """_hyper_key() by name: what decides the curve besides the data (the schedule as its descriptor (type, W, T) or None)."""
        return dict(zip(self.HYPER_NAMES, self._hyper_key()))

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
        if (bad or options_differ) and self._live_replays:
            import gc
            self.drop_captured_steps()
            gc.collect()
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
        eng = self.engine
        dev = eng.device
        copy_stream = torch.cuda.Stream(device=dev)
        # the slots (pinned host + device buffers) live as long as the trainer: a second pass over the same shapes re-uses them -- and, with
        # graphs=True, the steps captured over them
        skey = (int(sampler.S), int(sampler.max_pairs(MODE_TRAIN)), batch_size, depth)      # shapes, not id(sampler): an id can be re-used
        cache = self._live_slots
        if skey not in cache:
            sl = [sampler.alloc(batch_size, MODE_TRAIN, pinned=True) for _ in range(depth)]
            cache[skey] = (sl, [{k: torch.empty_like(v, device=dev) for k, v in s_.items()} for s_ in sl])
        slots, dslots = cache[skey]
        n = len(node_ids)
        t_sample, t_wait, t_copy = [0.0], [0.0], [0.0]

        def produce(step, slot, done):
            ts = time.perf_counter()
            if done is not None:
                done.synchronize()     # the slot (pinned + device buffers) may be refilled once the step that read it is done
            lo = (step * batch_size) % max(n - batch_size, 1)
            tg = np.resize(node_ids[lo:], batch_size)
            t1 = time.perf_counter()
            tgt, pair, num_pairs, labels = sampler.batch(tg, MODE_TRAIN, out=slots[slot], threads=threads,
                                                        base_seed=base_seed, counter=(first_step + step) * batch_size)
            t2 = time.perf_counter()
            P = int(pair["node_ids"].shape[0])
            d = dslots[slot]
            with torch.cuda.stream(copy_stream):
                for k, cnt in (("tgt_ids", batch_size), ("tgt_mask", batch_size), ("pair_ids", P), ("pair_mask", P),
                               ("num_pairs", batch_size), ("labels", P)):
                    d[k][:cnt].copy_(slots[slot][k][:cnt], non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            b = ({"node_ids": d["tgt_ids"][:batch_size], "attention_mask": d["tgt_mask"][:batch_size]},
                 {"node_ids": d["pair_ids"][:P], "attention_mask": d["pair_mask"][:P]}, d["num_pairs"][:batch_size], d["labels"][:P])
            t3 = time.perf_counter()
            t_wait[0] += t1 - ts
            t_sample[0] += t2 - t1
            t_copy[0] += t3 - t2
            return b, ev

        pipe = ProducerPipeline(produce, steps, depth, stall_timeout_s=stall_timeout_s)
        torch.cuda.synchronize()
        guarded = self._guard() is not None
        if guarded:
            count0 = eng.step_counters()               # the GPU is idle here
        t_start = time.perf_counter()
        t0 = None
        pipe.start()
        # GPU-side view of the pipeline: events around every step on the launch stream; the gap between one step's end and the
        # next step's start is time the GPU had nothing of this stream to run (input not there yet, or the launch thread late)
        ev_a = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
        ev_b = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
        t_launch = 0.0
        replays = self._live_replays       # (slot buffers, shape, hyper-parameters) -> captured step, kept across calls
        hyper = self._capture_key()
        if graphs and any(k[-1] != hyper for k in replays):
            self.drop_captured_steps()       # lr / weight decay / clip / ratios changed since the capture: those are frozen kernel arguments
        checked_at = -1
        try:
            for i, (slot, (b, ev)) in enumerate(pipe):
                if t0 is None:
                    t0 = time.perf_counter()       # sustained rate: the clock starts when the first batch is there (the fill is reported)
                tl = time.perf_counter()
                torch.cuda.current_stream().wait_event(ev)
                ev_a[i].record()
                key = (b[0]["node_ids"].data_ptr(), tuple(b[0]["node_ids"].shape), tuple(b[1]["node_ids"].shape), hyper) if graphs else None
                if graphs and self.check_carrier_every and self._opt_steps % self.check_carrier_every == 0 and self._opt_steps != checked_at:
                    # replays never run optimizer_step's Python-side guard: look at the LayerNorm parameters here (one small read per
                    # LayerNorm every N steps); when they no longer allow x^ from the LayerNorm output, the captured steps are dropped,
                    # the engine switches to stored inputs and the slots are captured again below
                    checked_at = self._opt_steps
                    if eng.carrier_needs_stored_inputs():
                        self.drop_captured_steps()
                        eng.check_layernorm_carrier()
                if graphs and key in replays:
                    self.last_loss = replays[key]()
                    self._opt_steps += 1
                elif graphs and self.world_size == 1 and self.accum == 1 and not self.force_exchange:
                    # first batch of this slot: record the step (nothing executes during capture), then replay it like every later one.
                    # thread_local: the producer thread keeps issuing its own copies / event waits while this thread captures
                    if replays and eng.carrier_needs_stored_inputs():
                        self.drop_captured_steps()       # (capture_step switches the option; it must not find live graphs then)
                    replays[key] = self.capture_step(b, warmup=0, capture_error_mode="thread_local")      # (counts one optimizer step: the recording)
                    self.last_loss = replays[key]()
                else:
                    self.train_step(b)
                ev_b[i].record()
                self.pipeline_step = first_step + i + 1
                pipe.release(slot, ev_b[i])   # the launch thread does not wait for the GPU: the producer does, before it refills
                t_launch += time.perf_counter() - tl
        finally:
            torch.cuda.synchronize()
            pipe.close()
        el = time.perf_counter() - t0
        extra = {}
        if guarded:
            count1 = eng.step_counters()               # the one read of the call's end, after its final synchronize
            extra["skipped_steps"] = count1["skipped"] - count0["skipped"]
            tried = count1["attempts"] - count0["attempts"]
            if self.step_log and 0 < tried <= self.step_log:
                extra["loss_train"] = [r["loss"] for r in eng.step_log() if r["attempt"] >= count0["attempts"]]
            self.check_nonfinite(count1)
        idle = sum(ev_b[i - 1].elapsed_time(ev_a[i]) for i in range(1, steps))
        busy = sum(ev_a[i].elapsed_time(ev_b[i]) for i in range(steps))
        return {"nodes_per_s": round(steps * batch_size / el, 1), "ms_per_step": round(el / steps * 1e3, 3),
                "pipeline_fill_ms": round((t0 - t_start) * 1e3, 3),
                "sampler_threads": threads, "steps": steps, "pipeline_depth": depth, "graph_replay": bool(graphs),
                "gpu_step_ms": round(busy / steps, 3),
                "gpu_idle_ms_per_step": round(idle / max(steps - 1, 1), 3),
                "launch_thread_busy_ms_per_step": round(t_launch / steps * 1e3, 3),
                "launch_thread_waiting_for_input_ms_per_step": round(pipe.starved_s / steps * 1e3, 3),
                "producer_ms_per_batch": {"sampling": round(t_sample[0] / steps * 1e3, 3), "h2d_issue": round(t_copy[0] / steps * 1e3, 3),
                                          "waiting_for_a_free_slot": round(t_wait[0] / steps * 1e3, 3)}, **extra}


class PipelineError(RuntimeError):
    """The producer thread of a ProducerPipeline died or stalled; the original exception (if any) is the __cause__."""


class ProducerPipeline:
    """`depth` reusable slots filled by ONE producer thread and drained in order by the calling thread (the host side of
    `Trainer.run_live`: sampler -> pinned slot -> async copy).  `produce(step, slot, token)` runs on the producer thread;
    `token` is whatever the consumer passed to `release(slot, token)` when it handed the slot back (None the first time).
    A producer that raises (sampler ValueError for an isolated / out-of-range node, a failed pin or copy) or stops
    delivering for `stall_timeout_s` does not leave the consumer blocked: iteration raises PipelineError instead."""

    def __init__(self, produce, steps: int, depth: int, stall_timeout_s: float = 120.0, poll_s: float = 0.2):
        self.produce, self.steps, self.depth = produce, steps, depth
        self.stall_timeout_s, self.poll_s = stall_timeout_s, poll_s
        self.free_q: "queue.Queue" = queue.Queue()
        self.ready_q: "queue.Queue" = queue.Queue()
        for i in range(depth):
            self.free_q.put((i, None))
        self.starved_s = 0.0
        self._stop = threading.Event()
        self._th = threading.Thread(target=self._run, daemon=True)

    def _run(self):
        try:
            for step in range(self.steps):
                while True:                      # a consumer that stopped early must not leave this thread blocked
                    if self._stop.is_set():
                        return
                    try:
                        slot, token = self.free_q.get(timeout=self.poll_s)
                        break
                    except queue.Empty:
                        continue
                self.ready_q.put(("item", slot, self.produce(step, slot, token)))
        except BaseException as exc:             # delivered to the consumer, which re-raises
            self.ready_q.put(("error", None, exc))

    def start(self):
        self._th.start()

    def release(self, slot: int, token=None):
        self.free_q.put((slot, token))

    def close(self):
        self._stop.set()
        if self._th.is_alive():
            self._th.join(timeout=5.0)

    def __iter__(self):
        for _ in range(self.steps):
            t0 = time.perf_counter()
            while True:
                try:
                    kind, slot, payload = self.ready_q.get(timeout=self.poll_s)
                    break
                except queue.Empty:
                    waited = time.perf_counter() - t0
                    if not self._th.is_alive() and self.ready_q.empty():
                        raise PipelineError("input pipeline: the producer thread exited without delivering a batch")
                    if waited > self.stall_timeout_s:
                        raise PipelineError(f"input pipeline: no batch for {waited:.0f} s (producer stalled)")
            self.starved_s += time.perf_counter() - t0
            if kind == "error":
                raise PipelineError(f"input pipeline: producer failed: {payload!r}") from payload
            yield slot, payload


def roc_auc_score(labels: np.ndarray, scores: np.ndarray) -> float:
    """sklearn.metrics.roc_auc_score for binary labels (what `_valid_and_test_epoch_end` logs as val/auc,
    pmgt/pmgt/trainer.py:182-195): Mann-Whitney U with midranks for ties."""
    labels = np.asarray(labels).astype(bool)
    scores = np.asarray(scores, dtype=np.float64)
    n_pos, n_neg = int(labels.sum()), int((~labels).sum())
    if n_pos == 0 or n_neg == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    order = np.argsort(scores, kind="mergesort")
    s = scores[order]
    ranks = np.empty(len(s), dtype=np.float64)
    i = 0
    while i < len(s):
        j = i
        while j + 1 < len(s) and s[j + 1] == s[i]:
            j += 1
        ranks[i:j + 1] = 0.5 * (i + j) + 1.0
        i = j + 1
    r = np.empty_like(ranks)
    r[order] = ranks
    return float((r[labels].sum() - n_pos * (n_pos + 1) / 2.0) / (n_pos * n_neg))


EVAL_PINNED_SLOTS = 4      # evaluate(metrics="device"): pinned batch buffers in flight


def _evaluate_device(engine, sampler, mine: np.ndarray, batch_size: int, threads: int, seed: int, rank: int, ws: int):
    """evaluate(metrics="device"): the same batches through pinned host buffers and non-blocking copies, scores / labels / loss kept on the
    device by a ValidationMetrics.  Nothing in the loop waits for the GPU's compute, so the sampler call of batch k + 1 runs while the GPU
    works on batch k.  The pinned buffers form a ring of EVAL_PINNED_SLOTS: before the sampler overwrites a slot, the host waits for the
    event behind THAT slot's own copies, EVAL_PINNED_SLOTS batches back -- back-pressure that bounds the run-ahead, not a per-batch sync."""
    from .metrics import ValidationMetrics
    dev = engine.device
    vm = ValidationMetrics(dev, max(len(mine) * max(sampler.max_pairs(MODE_EVAL), 1), 1))
    rows = max(min(int(batch_size), len(mine)), 1)
    ring = [dict(buf=sampler.alloc(rows, MODE_EVAL, pinned=True), copied=None) for _ in range(EVAL_PINNED_SLOTS)]
    for k, lo in enumerate(range(0, len(mine), batch_size)):
        tg = mine[lo: lo + batch_size]
        slot = ring[k % EVAL_PINNED_SLOTS]
        if slot["copied"] is not None:
            slot["copied"].synchronize()
        tgt, pair, num_pairs, labels = sampler.batch(tg, MODE_EVAL, out=slot["buf"], threads=threads, base_seed=seed, counter=rank + ws * lo,
                                                      counter_stride=ws)
        cu = lambda d: {k_: v.to(dev, non_blocking=True) for k_, v in d.items()}
        labels_dev = labels.to(dev, non_blocking=True)
        batch = (cu(tgt), cu(pair), num_pairs.to(dev, non_blocking=True), labels_dev)
        slot["copied"] = torch.cuda.Event()
        slot["copied"].record()
        out = engine.pretrain_step(batch, training=False, want_hidden=False)
        vm.update(out["logits"], labels_dev, out["loss"], len(tg))
    n_total = len(mine)
    if ws > 1:
        import torch.distributed as dist
        preds, labs = gather_predictions(vm.scores(), vm.labels())       # one transfer per validation, not one per batch
        parts = [None] * ws
        dist.all_gather_object(parts, (vm.loss_sum(), n_total))
        loss_sum, n_total = sum(p[0] for p in parts), sum(p[1] for p in parts)
        vm = ValidationMetrics(dev, max(len(preds), 1))
        if len(preds):
            vm.update_scores(torch.from_numpy(preds).to(dev), torch.from_numpy(labs).to(dev))
        return {"loss/val": float(loss_sum / max(n_total, 1)), "val/auc": vm.result()["val/auc"]}
    return vm.result()


@torch.no_grad()
def evaluate(engine, sampler, node_ids: np.ndarray, batch_size: int = 256, threads: int = 8, seed: int = 0,
             distributed: bool = False, metrics: str = "host"):
    """Validation pass (pmgt/pmgt/trainer.py:162-195): eval-mode forward with 1 positive + 1 negative
    per target, sigmoid(logits) vs labels -> {'loss/val', 'val/auc'}.  `loss/val` is the mean of the per-batch losses
    (what `self.log("loss/val", ...)` aggregates over an epoch, weighted by batch size).  distributed=True under an
    initialised process group: rank r evaluates node_ids[r::W] and the predictions of all ranks are gathered, so every
    rank reports the same AUC over the whole validation set (the reference's AUC is per rank: no sync_dist); every node
    draws from the stream of its GLOBAL index, so the result equals the single-process evaluation of the same list.
    metrics="host" (default): predictions and the loss are copied to the host after every batch and roc_auc_score runs there.
    metrics="device": they stay on the device (pmgt_amd.metrics.ValidationMetrics: sigmoid, loss accumulation, sort and the Mann-Whitney
    statistic in HIP) and one small copy at the end fetches the result; `loss/val` is bit-identical to the host path, `val/auc` is
    roc_auc_score of the scores the device computed, exactly (its sigmoid may differ from torch's in the last bit)."""
    if metrics not in ("host", "device"):
        raise ValueError(f"metrics={metrics!r}: expected 'host' or 'device'")
    node_ids = np.asarray(node_ids)
    rank, ws = world() if distributed else (0, 1)
    mine = node_ids[rank::ws]
    if metrics == "device":
        return _evaluate_device(engine, sampler, mine, batch_size, threads, seed, rank, ws)
    preds, labs = [np.empty(0, np.float32)], [np.empty(0, np.float32)]
    loss_sum = 0.0
    for lo in range(0, len(mine), batch_size):
        tg = mine[lo: lo + batch_size]
        tgt, pair, num_pairs, labels = sampler.batch(tg, MODE_EVAL, threads=threads, base_seed=seed, counter=rank + ws * lo,
                                                      counter_stride=ws)      # item j of this rank = item rank + ws * j of the list
        cu = lambda d: {k: v.to(engine.device) for k, v in d.items()}
        out = engine.pretrain_step((cu(tgt), cu(pair), num_pairs.to(engine.device), labels.to(engine.device)),
                                   training=False, want_hidden=False)
        preds.append(torch.sigmoid(out["logits"]).cpu().numpy())
        labs.append(labels.numpy())
        loss_sum += out["loss"].item() * len(tg)
    preds, labs = np.concatenate(preds), np.concatenate(labs)
    n_total = len(mine)
    if ws > 1:
        import torch.distributed as dist
        preds, labs = gather_predictions(preds, labs)
        parts = [None] * ws
        dist.all_gather_object(parts, (loss_sum, n_total))
        loss_sum, n_total = sum(p[0] for p in parts), sum(p[1] for p in parts)
    return {"loss/val": float(loss_sum / max(n_total, 1)), "val/auc": roc_auc_score(labs, preds)}


@torch.no_grad()
def export_embeddings(engine, sampler, n_nodes: int, batch_size: int = 1024, threads: int = 8, seed: int = 0) -> np.ndarray:
    """Inference / export (pmgt/pmgt/trainer.py:153-154,259-275; pmgt/base_trainer.py:400-407): CLS hidden
    state of every node in id order as fp32 [N, d] (contexts are still randomly sampled, as in the reference)."""
    out = np.empty((n_nodes, engine.config.hidden_size), dtype=np.float32)
    ids = np.arange(2, n_nodes + 2)
    for lo in range(0, n_nodes, batch_size):
        tg = ids[lo: lo + batch_size]
        tgt = sampler.batch(tg, MODE_INFERENCE, threads=threads, base_seed=seed, counter=lo)
        last, _, _ = engine.encode(ids=tgt["node_ids"].to(engine.device), attention_mask=tgt["attention_mask"].to(engine.device))
        out[lo: lo + len(tg)] = last[:, 0].float().cpu().numpy()
    return out


# ================================================================================================
# fit: the reference's driver (pmgt/base_trainer.py:283-336: pl.Trainer.fit with max_epochs, validation every epoch,
# EarlyStopping(monitor, patience, mode), ModelCheckpoint(save_top_k=1, save_last=True), resume through ckpt_path)
# ================================================================================================
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
        import os
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
    from .parallel import shard_indices
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
    import os

    from . import io as pio
    eng = trainer.engine
    if getattr(model_or_engine, "engine", model_or_engine) is not eng:
        raise ValueError("fit: the trainer drives another engine than the one passed")
    if eval_metrics not in ("host", "device"):
        raise ValueError(f"eval_metrics={eval_metrics!r}: expected 'host' or 'device'")
    passed = {k: v for k, v in (("nonfinite", nonfinite), ("step_log", step_log), ("max_skipped_in_a_row", max_skipped_in_a_row)) if v != "keep"}
    if passed:
        checked = Trainer(None, **passed)                 # the constructor's argument checks
        for k in passed:
            setattr(trainer, k, getattr(checked, k))      # (run_live re-captures: both settings are part of _hyper_key())
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
            tgt, pair, num_pairs, labels = sampler.batch(order[n_full * batch_size:], MODE_TRAIN, threads=threads, base_seed=stream_seed,
                                                          counter=trainer.pipeline_step * batch_size)
            cu = lambda d: {k_: v.to(eng.device) for k_, v in d.items()}
            trainer.train_step((cu(tgt), cu(pair), num_pairs.to(eng.device), labels.to(eng.device)))
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
        import contextlib
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
