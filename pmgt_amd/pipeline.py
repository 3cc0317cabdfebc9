"""The live input pipeline: threaded C++ MCNSampling -> pinned buffers -> side-stream H2D -> the training step.  `ProducerPipeline` is the
host side (one producer thread, reusable slots), `live_loop` the loop behind `Trainer.run_live`, which states its contract."""
import queue
import threading
import time

import numpy as np
import torch

from .datasets import MODE_TRAIN


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


def _slots(trainer, sampler, batch_size: int, depth: int):
    """The pinned host slots and their device buffers, kept with the trainer: a second pass over the same shapes re-uses them and their captures."""
    skey = (int(sampler.S), int(sampler.max_pairs(MODE_TRAIN)), batch_size, depth)      # shapes, not id(sampler): an id can be re-used
    cache = trainer._live_slots
    if skey not in cache:
        sl = [sampler.alloc(batch_size, MODE_TRAIN, pinned=True) for _ in range(depth)]
        cache[skey] = (sl, [{k: torch.empty_like(v, device=trainer.engine.device) for k, v in s_.items()} for s_ in sl])
    return cache[skey]


def _producer(sampler, node_ids, batch_size: int, slots, dslots, copy_stream, threads: int, base_seed: int, first_step: int):
    """`produce` of the ProducerPipeline (sampler call into a pinned slot, its async H2D copies on `copy_stream`) and the seconds each part took."""
    n = len(node_ids)
    spent = {"sampling": 0.0, "h2d_issue": 0.0, "waiting_for_a_free_slot": 0.0}

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
        spent["waiting_for_a_free_slot"] += t1 - ts
        spent["sampling"] += t2 - t1
        spent["h2d_issue"] += t3 - t2
        return b, ev
    return produce, spent


def _stepper(trainer, graphs: bool):
    """step(b) of the launch thread: the eager step or, with graphs=True, replay / capture then replay / eager where the step is not capturable."""
    replays = trainer._live_replays       # (slot buffers, shape, hyper-parameters) -> captured step, kept across calls
    hyper = trainer._capture_key()
    if graphs and any(k[-1] != hyper for k in replays):
        trainer.drop_captured_steps()       # lr / weight decay / clip / ratios changed since the capture: those are frozen kernel arguments
    if not graphs:
        return trainer.train_step
    checked_at = -1

    def step(b):
        nonlocal checked_at
        key = (b[0]["node_ids"].data_ptr(), tuple(b[0]["node_ids"].shape), tuple(b[1]["node_ids"].shape), hyper)
        if trainer.check_carrier_every and trainer._opt_steps % trainer.check_carrier_every == 0 and trainer._opt_steps != checked_at:
            # replays never run optimizer_step's Python-side guard: look at the LayerNorm parameters here (one small read per
            # LayerNorm every N steps); when they no longer allow x^ from the LayerNorm output, the captured steps are dropped,
            # the engine switches to stored inputs and the slots are captured again below
            checked_at = trainer._opt_steps
            trainer._check_carrier()
        if key in replays:
            trainer.last_loss = replays[key]()
            trainer._opt_steps += 1
        elif trainer._capturable:
            # first batch of this slot: record the step (nothing executes during capture), then replay it like every later one.
            # thread_local: the producer thread keeps issuing its own copies / event waits while this thread captures
            if replays:
                trainer._check_carrier()       # (capture_step switches the option; it must not find live graphs then)
            replays[key] = trainer.capture_step(b, warmup=0, capture_error_mode="thread_local")      # (counts one optimizer step: the recording)
            trainer.last_loss = replays[key]()
        else:
            trainer.train_step(b)
    return step


def _report(steps, batch_size, threads, depth, graphs, el, fill_s, ev_a, ev_b, t_launch, starved_s, spent, extra) -> dict:
    """What run_live returns: the sustained rate, the GPU-side view from the events around every step, and where both host threads' time went."""
    idle = sum(ev_b[i - 1].elapsed_time(ev_a[i]) for i in range(1, steps))
    busy = sum(ev_a[i].elapsed_time(ev_b[i]) for i in range(steps))
    return {"nodes_per_s": round(steps * batch_size / el, 1), "ms_per_step": round(el / steps * 1e3, 3),
            "pipeline_fill_ms": round(fill_s * 1e3, 3),
            "sampler_threads": threads, "steps": steps, "pipeline_depth": depth, "graph_replay": bool(graphs),
            "gpu_step_ms": round(busy / steps, 3),
            "gpu_idle_ms_per_step": round(idle / max(steps - 1, 1), 3),
            "launch_thread_busy_ms_per_step": round(t_launch / steps * 1e3, 3),
            "launch_thread_waiting_for_input_ms_per_step": round(starved_s / steps * 1e3, 3),
            "producer_ms_per_batch": {k: round(v / steps * 1e3, 3) for k, v in spent.items()}, **extra}


def live_loop(trainer, sampler, node_ids, batch_size, steps, threads, depth, stall_timeout_s, graphs, first_step, base_seed) -> dict:
    """The body of Trainer.run_live, whose signature and docstring state the contract."""
    eng = trainer.engine
    copy_stream = torch.cuda.Stream(device=eng.device)
    slots, dslots = _slots(trainer, sampler, batch_size, depth)
    produce, spent = _producer(sampler, node_ids, batch_size, slots, dslots, copy_stream, threads, base_seed, first_step)
    pipe = ProducerPipeline(produce, steps, depth, stall_timeout_s=stall_timeout_s)
    torch.cuda.synchronize()
    guarded = trainer._guard() is not None
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
    step = _stepper(trainer, graphs)
    try:
        for i, (slot, (b, ev)) in enumerate(pipe):
            if t0 is None:
                t0 = time.perf_counter()       # sustained rate: the clock starts when the first batch is there (the fill is reported)
            tl = time.perf_counter()
            torch.cuda.current_stream().wait_event(ev)
            ev_a[i].record()
            step(b)
            ev_b[i].record()
            trainer.pipeline_step = first_step + i + 1
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
        if trainer.step_log and 0 < tried <= trainer.step_log:
            extra["loss_train"] = [r["loss"] for r in eng.step_log() if r["attempt"] >= count0["attempts"]]
        trainer.check_nonfinite(count1)
    return _report(steps, batch_size, threads, depth, graphs, el, t0 - t_start, ev_a, ev_b, t_launch, pipe.starved_s, spent, extra)
