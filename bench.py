#!/usr/bin/env python3
"""PMGT pre-training throughput on MI355X (BASELINE.json metric: target nodes/sec).

One "step" = one full pre-training step of the hot path on one batch of B target nodes per GPU
(12 sequences of S tokens per target: target + 10 pairs + masked copy): device NFR masking, batched
encoder forward, GSR + NFR losses, backward, [RCCL gradient all-reduce when N > 1], global-norm clip +
AdamW.  Inputs (sampled node-context batches, feature tables) are resident in HBM before the timed
region.  Workload at N=1: BASELINE.json configs[1] — VG-sized synthetic item graph (7 252 nodes /
88 606 edges), L=4 H=8 d=256 I=256 S=32, bf16, B=1024 targets/GPU/step, dropout 0.1, lr 1e-4, wd 1e-2, clip 5.0.

Prints ONE JSON line (rank 0).  N > 1: one process per GPU -- either launched by torch.distributed.run (the driver's
form: WORLD_SIZE / RANK / LOCAL_RANK in the environment, `--gpus` must equal WORLD_SIZE), or `python bench.py --gpus N` alone:
with WORLD_SIZE unset this process starts the N ranks itself (torch.distributed.run as a child, before anything here touches
the GPU) and exits with their status -- what `pl.Trainer(gpus=N)` does for the reference (pmgt/base_trainer.py:309-322).

A plain run sets up, warms up, times --steps steps and prints the line.  --full adds the side measurements after the timed steps (host
sampler rate, per-phase pass with rooflines, batch sweep, live pipeline, child workloads, CPU baseline, all-reduce timing); none of
them changes `value` or `ms_per_step`.  --dump-outputs DIR writes what the last timed step computed as .npy files, for comparing builds.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # MI355X_MICROARCH.md: 8 TB/s spec
MFMA_BF16_PEAK_TFLOPS = 2500.0   # dense bf16 (never the 2:1-sparse figure)
MFMA_F32_PEAK_TFLOPS = 157.3

WORKLOADS = {
    # name: (nodes, edges, L, H, d, I, S)
    "c1": (7252, 88606, 2, 4, 128, 128, 16),
    "c2": (7252, 88606, 4, 8, 256, 256, 32),
    "c3": (10834, 38252, 4, 8, 256, 256, 32),
    "c4": (1000000, 20000000, 6, 8, 512, 512, 64),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--workload", default="c2", choices=sorted(WORKLOADS))
    ap.add_argument("--batch", type=int, default=1024,
                    help="target nodes per GPU per step; SURVEY 8(d) lists 32 (author's script), 256 (CLI default), 1024")
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "fp32", "fp8"],
                    help="bf16 = BASELINE.json's metric; fp8 = bf16 engine with e4m3 feature tables / fp8-MFMA feature + Q|K|V|C projections (config 5)")
    ap.add_argument("--dropout", type=float, default=0.1)
    ap.add_argument("--intermediate", type=int, default=0, help="override intermediate size")
    ap.add_argument("--beta", type=float, default=0.5,
                    help="PMGTConfig.beta (default 0.5 = the config default, configuration_pmgt.py:21); 1.0 = the author's script (scripts/run_pmgt.sh:24): "
                         "the dot-product branch is dead and the fused kernels skip Q / K altogether")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-phase-profile", action="store_true")
    ap.add_argument("--overlap", action="store_true", help="partial-sum reductions on the engine's side stream (A/B; measured neutral)")
    ap.add_argument("--sampler-threads", type=int, default=0)
    ap.add_argument("--end-to-end", action="store_true", help="N = 1: on by default; N > 1: also time steps fed by the live host sampler on every rank")
    ap.add_argument("--no-end-to-end", action="store_true", help="skip the live-sampler pass")
    ap.add_argument("--no-batch-sweep", action="store_true", help="skip the B=32 / B=256 extra measurements (N=1 only)")
    # default "two" (= Trainer's default; provisional until a multi-GPU A/B exists -- at N = 8 try "one" next: 12.2 MB is a bandwidth-sized
    # message over seven xGMI links, and "layer" for the most overlap): one-rank RCCL runs (profiles/r05/rccl_single_rank_exchange.txt) put six per-bucket collectives at +2.5 % of the step, two at
    # +1.8 %; the first of the two (9.8 MB: NFR head + layers) travels under the embedding backward, only the 2.5 MB embedding bucket is exposed
    ap.add_argument("--buckets", default="two", choices=["layer", "two", "one"],
                    help="N > 1: gradient all-reduce per engine bucket (NFR head, each layer, embeddings), as two collectives "
                         "(head + encoder layers | embeddings), or as one after the backward pass")
    ap.add_argument("--engine-option", action="append", default=[], metavar="KEY",
                    help="A/B: set a path option of the engine (include/pmgt_ops.h, e.g. no_role_split_ln); repeatable; reported in the line")
    ap.add_argument("--no-extra-workloads", action="store_true",
                    help="skip the c4 (bf16) / c5 (fp8) lines the default N = 1 run appends under \"workloads\" (child processes)")
    ap.add_argument("--force-exchange", action="store_true",
                    help="N = 1: initialise a ONE-rank nccl (= RCCL) process group and run the N > 1 code path unchanged on it -- AVG probe, "
                         "bucketed async all-reduce from the engine's gradient-ready callback, wait in front of the optimizer, the "
                         "allreduce measurement, barrier, destroy: RCCL executes the exchange on a one-GPU box")
    ap.add_argument("--detail-out", default="", metavar="PATH",
                    help="where the full record goes (phases, top-3 rooflines, sweeps, per-child detail); default bench_detail.json next to this "
                         "script (+ a copy under gpurun_out/ when that directory exists).  stdout carries ONE compact line of at most 4 KB")
    ap.add_argument("--rehearse-launch", action="store_true",
                    help="launcher check that needs no GPU: the ranks rendezvous over gloo, all-reduce their ranks and rank 0 prints "
                         "a line with n_gpus = world and value = null")
    ap.add_argument("--full", action="store_true",
                    help="also run the side measurements after the timed steps: host sampler rate, phase pass + rooflines, batch sweep, live "
                         "pipeline, child workloads, CPU baseline, all-reduce timing (each still switched off by its --no-* option).  Without "
                         "it a run sets up, warms up, times --steps steps and prints the line")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="after the timed steps, write what the last timed step computed (losses, logits, masked-row count, pre-clip "
                         "gradient norm, gradients, updated parameters) as DIR/<name>.npy in float32 / float64, at most 64 MB in all")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


def spawn_ranks(args):
    """`python bench.py --gpus N` with no launcher around it: start N rank processes (torch.distributed.run, rendezvous on
    127.0.0.1) running this same command line and return their exit status.  Called before any GPU call of this process: the
    parent only waits."""
    import socket
    import subprocess
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.run(cmd, env=env).returncode


def rehearse_launch(world, rank):
    """No GPU: proves the launch path (rank environment, rendezvous, a collective, symmetric teardown, one line from rank 0)."""
    import torch.distributed as dist
    dist.init_process_group("gloo")
    t = torch.tensor([float(rank)])
    dist.all_reduce(t)
    dist.barrier()
    if rank == 0:
        print(json.dumps({"metric": "PMGT pre-train nodes/sec", "value": None, "unit": "target nodes/s", "n_gpus": world,
                          "rehearsal": "launch only (gloo, no GPU)", "rank_sum": t.item()}))
    dist.barrier()
    dist.destroy_process_group()


def phase_work(name, M, d, I, S, H, Fv, Ft, cap_rows, esz, vc=False):
    """Algorithmic (flops, bytes) of ONE launch group of a phase, for the roofline object.
    M = tokens in the step, esz = bytes per activation element."""
    F = Fv + Ft
    g = lambda m, n, k: 2.0 * m * n * k
    table = {
        "fwd.gemm_featproj": (g(M, d, F) / 2, M * F / 2 * esz + M * d * esz),   # two launches: avg of (Fv, Ft)
        "fwd.gemm_qkvc": (g(M, 4 * d, d), M * 5 * d * esz),
        "fwd.gemm_attn_out": (g(M, d, d), M * 3 * d * esz),
        "fwd.gemm_ffn1": (g(M, I, d), M * (d + 2 * I) * esz),
        "fwd.gemm_ffn2": (g(M, d, I), M * (I + 2 * d) * esz),
        "fwd.attention": (6.0 * M * S * d, M * 5 * d * esz),
        # fused projection + attention: reads x (1U), writes Q|K|V|C (4U, kept for the backward) and ctx (1U)
        "fwd.qkvc_attention": (g(M, 4 * d, d) + 6.0 * M * S * d, M * 6 * d * esz),
        "bwd.attention": (16.0 * M * S * d, M * 9 * d * esz),
        # attention backward fused with the Q|K|V|C weight gradient: reads Q|K|V|C (4U), dctx (1U), x (1U), writes dQ|dK|dV|dC (4U);
        # it runs on L - 1 layers (the last one takes the CLS-only shortcut through the two separate kernels): M of ONE launch
        "bwd.attention_wgrad": (16.0 * M * S * d + g(M, 4 * d, d), M * 10 * d * esz),
        "bwd.dgrad_ffn2": (g(M, I, d), M * (d + 2 * I) * esz),
        "bwd.dgrad_ffn1": (g(M, d, I), M * (I + 2 * d) * esz),
        "bwd.dgrad_attn_out": (g(M, d, d), M * 2 * d * esz),
        "bwd.dgrad_qkvc": (g(M, d, 4 * d), M * 6 * d * esz),
        # the same GEMMs with the LayerNorm backward of their result as epilogue (dy never stored): + y in, dx and dx_drop out
        "bwd.dgrad_ffn1_lnb": (g(M, d, I), M * (I + 4 * d) * esz),
        "bwd.dgrad_qkvc_lnb": (g(M, d, 4 * d), M * 8 * d * esz),
        "bwd.wgrad_ffn2": (g(M, d, I), M * (d + I) * esz),
        "bwd.wgrad_ffn1": (g(M, I, d), M * (d + I) * esz),
        "bwd.wgrad_attn_out": (g(M, d, d), M * 2 * d * esz),
        "bwd.wgrad_qkvc": (g(M, 4 * d, d), M * 5 * d * esz),
        "bwd.wgrad_featproj": (g(M, d, F) / 2, M * (d + F / 2) * esz),
        "fwd.layernorm": (0.0, M * 2 * d * esz),
        "bwd.layernorm": (0.0, M * 4 * d * esz),
        "fwd.embed_mix": (0.0, M * 4 * d * esz),
        "bwd.embed_mix": (0.0, M * 7 * d * esz),
    }
    if vc:      # beta == 1 with the dead branch skipped: V | C only (2 d columns instead of 4 d), the cosine branch alone
        table["fwd.qkvc_attention"] = (g(M, 2 * d, d) + 3.0 * M * S * d, M * 4 * d * esz)                      # x in, V | C + ctx out
        table["bwd.attention_wgrad"] = (8.0 * M * S * d + g(M, 2 * d, d), M * 6 * d * esz)                     # V | C, d ctx, x in; dV | dC out
        table["bwd.dgrad_qkvc"] = (g(M, d, 2 * d), M * 4 * d * esz)
        table["bwd.dgrad_qkvc_lnb"] = (g(M, d, 2 * d), M * 6 * d * esz)
    return table.get(name)


DEFAULT_BATCH = {"c4": 256}      # the batch a workload's bench lines quote (everything else: 1 024)


def traffic_key(workload, intermediate, beta, batch=None):
    """Name of the committed PMC summary (profiles/traffic[_<key>].json) that belongs to a bench configuration."""
    b = "" if batch is None or batch == DEFAULT_BATCH.get(workload, 1024) else f"_b{batch}"
    return workload + (f"_i{intermediate}" if intermediate else "") + ("_beta1" if beta == 1.0 else "") + b


def dead_branch_skipped(args, d, H, S):
    """beta == 1 and the shapes the V | C-only kernels take (engine.hip vc_only_applies)."""
    return (args.beta == 1.0 and args.dtype == "bf16" and S == 32 and d // H == 32 and H % 4 == 0
            and "no_beta_skip" not in args.engine_option)


def host_cpu_share():
    """CPUs this process may actually use: the cgroup CPU quota when there is one (a GPU box shows all 256 hardware threads
    in os.cpu_count() but grants a share of them), else the affinity mask."""
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            return float(quota) / float(period)
    except (OSError, ValueError):
        pass
    try:
        q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        if q > 0:
            return q / per
    except (OSError, ValueError):
        pass
    try:
        return float(len(os.sched_getaffinity(0)))
    except AttributeError:
        return float(os.cpu_count() or 1)


def kernel_sources_sha():
    """Fingerprint of the HIP sources: profiles/traffic.json is only quoted when it was measured on these kernels."""
    import hashlib
    h = hashlib.sha256()
    csrc = os.path.join(ROOT, "pmgt_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".hip", ".h")):
            h.update(f.encode())
            h.update(open(os.path.join(csrc, f), "rb").read())
    return h.hexdigest()[:16]


def clock_probe(n_blocks=64):
    """{cycles, wall ticks, XCC} samples of the library's probe kernel on the current stream (device tensor; read it after a sync)."""
    import ctypes as C
    from pmgt_amd import _lib
    out = torch.zeros(n_blocks, 4, dtype=torch.int64, device="cuda")
    _lib.check(_lib.hip().pmgt_op_clock_probe(C.c_void_p(out.data_ptr()), n_blocks, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
    return out


def sustained_sclk_mhz(before, after):
    """Shader clock between two probes: per XCC, (cycle counter difference) / (100 MHz wall counter difference); median over the XCCs."""
    a, b = before.cpu().numpy(), after.cpu().numpy()
    per = []
    for x in sorted(set(a[:, 2].tolist()) & set(b[:, 2].tolist())):
        ra, rb = a[a[:, 2] == x][0], b[b[:, 2] == x][0]
        if rb[1] > ra[1]:
            per.append(float(rb[0] - ra[0]) / (float(rb[1] - ra[1]) / 100.0))
    return round(float(np.median(per)), 1) if per else None


def time_steps(trainer, staged, steps, warmup):
    for i in range(warmup):
        trainer.train_step(staged[i % len(staged)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(steps):
        trainer.train_step(staged[(warmup + i) % len(staged)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps


DUMP_BUDGET = 60_000_000     # bytes of .npy payload per --dump-outputs directory (64 MB with room for the file headers)
DUMP_WHOLE = 1 << 20         # arrays up to this size are always written whole


def last_step_outputs(trainer, eng):
    """What the last train_step handed its caller (the engine's output set of that step) and left in the engine (gradients, parameters
    after clip + AdamW), as host arrays.  Call before any further step: the output set is recycled."""
    o = trainer.last_outputs
    return {"losses": o["losses"].float().cpu().numpy(),                     # [loss, GSR loss, NFR loss]
            "logits": o["logits"].float().cpu().numpy(),
            "nfr_count": o["nfr_count"].cpu().numpy().astype(np.float64),
            "grad_norm": eng.grad_norm().reshape(1).float().cpu().numpy(),
            "grads": eng.grads.float().cpu().numpy(),
            "params": eng.params.float().cpu().numpy()}


def dump_outputs(dirname, arrays, budget=DUMP_BUDGET):
    """arrays -> dirname/<name>.npy (1-D, float32 / float64).  Arrays above DUMP_WHOLE share what the small ones leave of `budget`; one
    that does not fit its share is written as a fixed sample: the elements at a sorted draw without replacement from a generator
    seeded with 0, so two runs of the same configuration write the same positions."""
    os.makedirs(dirname, exist_ok=True)
    flat = {k: np.ascontiguousarray(v).reshape(-1) for k, v in arrays.items()}
    small = sum(a.nbytes for a in flat.values() if a.nbytes <= DUMP_WHOLE)
    n_big = sum(1 for a in flat.values() if a.nbytes > DUMP_WHOLE)
    share = (budget - small) // max(n_big, 1)
    for k, a in flat.items():
        if a.nbytes > DUMP_WHOLE and a.nbytes > share:
            keep = share // a.itemsize
            a = a[np.sort(np.random.default_rng(0).choice(a.size, keep, replace=False))]
        np.save(os.path.join(dirname, k + ".npy"), a)


def main():
    args = parse()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(spawn_ranks(args))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        sys.exit(f"bench.py: --gpus {args.gpus} but the launcher started WORLD_SIZE={world} ranks: refusing to report a line "
                 f"for a different GPU count than was asked for")
    if args.rehearse_launch:
        return rehearse_launch(world, rank)
    exchange = world > 1 or args.force_exchange
    line_out = sys.stdout
    if exchange:
        # RCCL prints a version banner to the C-level stdout when its first communicator comes up ("RCCL version : ..."): everything any library
        # writes to file descriptor 1 goes to stderr from here on, the ONE JSON line goes to the real stdout through a duplicate kept aside
        sys.stdout.flush()
        line_out = os.fdopen(os.dup(1), "w")
        os.dup2(2, 1)
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        own_store = None
        if world == 1 and "MASTER_PORT" not in os.environ:
            # --force-exchange without a launcher: a one-rank rendezvous of our own through a file (no port to find, so no window in which
            # another process of a shared host can take it)
            import tempfile
            own_store = dist.FileStore(os.path.join(tempfile.mkdtemp(prefix="pmgt_bench_store_"), "store"), 1)
        # rehearsal of the N > 1 control flow on a one-GPU box: PMGT_BENCH_BACKEND=gloo PMGT_BENCH_ONE_DEVICE=1 (every rank
        # on cuda:0, gradients all-reduced through the host); the driver's runs use the defaults (RCCL, one GPU per rank)
        backend = os.environ.get("PMGT_BENCH_BACKEND", "nccl")
        if os.environ.get("PMGT_BENCH_ONE_DEVICE") == "1":
            local = 0
        torch.cuda.set_device(local)
        kw = {"store": own_store, "rank": 0, "world_size": 1} if own_store is not None else {}
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device(f"cuda:{local}"), **kw)
        else:
            dist.init_process_group(backend, **kw)
    dev = f"cuda:{local}"

    from pmgt_amd.configuration_pmgt import PMGTConfig
    from pmgt_amd.datasets import MODE_TRAIN, MCNSampler
    from pmgt_amd.engine import Engine
    from pmgt_amd.graph import synthetic_graph
    from pmgt_amd.models import encoder_flops_per_node, executed_flops_per_node, reference_init, synthetic_features, train_flops_per_node
    from pmgt_amd.trainer import Trainer

    nodes, edges, L, H, d, I, S = WORKLOADS[args.workload]
    if args.intermediate:
        I = args.intermediate
    B = args.batch
    cfg = PMGTConfig(hidden_size=d, num_hidden_layers=L, num_attention_heads=H, intermediate_size=I,
                     hidden_dropout_prob=args.dropout, attention_probs_dropout_prob=args.dropout, beta=args.beta)
    t_setup = time.perf_counter()
    big = nodes >= 500_000
    if big:
        # million-node shapes: the circulant construction (seconds; the G(n, m) one sorts 4 x 10^7 keys four times: two minutes) and
        # feature tables drawn on the device (3.5 x 10^9 normals: another two minutes on one host core)
        from pmgt_amd.graph import synthetic_graph_regular
        graph = synthetic_graph_regular(nodes, edges, seed=0)
        gen = torch.Generator(device=dev).manual_seed(0)
        feats = []
        for f in (1536, 768):
            a = torch.randn(nodes + 2, f, generator=gen, device=dev, dtype=torch.float32)
            a[:2] = 0
            feats.append(a if args.dtype == "fp8" else a.to(torch.bfloat16 if args.dtype == "bf16" else torch.float32))
            del a
        vis, txt = feats
        del feats
    else:
        graph = synthetic_graph(nodes, edges, seed=0)
        vis, txt = synthetic_features(nodes, seed=0)
    eng = Engine(cfg, dtype=args.dtype, device=dev, seed=1234)
    if args.overlap:
        eng.set_overlap(True)
    for key in args.engine_option:
        eng.set_option(key, 1)
    reference_init(eng, seed=0)
    eng.set_tables(vis, txt)
    del vis, txt
    trainer = Trainer(eng, lr=1e-4, weight_decay=1e-2, max_grad_norm=5.0, world_size=world, buckets=args.buckets,
                      force_exchange=args.force_exchange and world == 1)
    trainer.broadcast_parameters()

    # ---- pre-stage node-context batches in HBM (host MCNSampling, C++ worker pool)
    from pmgt_amd.parallel import shard_indices
    share = host_cpu_share()
    local_world = int(os.environ.get("LOCAL_WORLD_SIZE", str(world)))
    # sampler workers per rank: this rank's part of the CPU share minus three CPUs for the launch thread, the producer thread and the runtime's
    # (three, not two: tools/e2e_sweep.py on a 16-CPU share -- 13 workers leave the launch thread, the producer thread and the HIP runtime's
    #  own threads a CPU each; with 14 the sampler is 5 % faster per batch and the pipeline no better)
    threads = args.sampler_threads or int(max(2, min(32, share / max(local_world, 1) - 3)))
    sampler = MCNSampler(graph, max_ctx_neigh=S - 1)
    # DistributedSampler semantics (what PL injects, pmgt/base_trainer.py:309-322): rank r takes r::W of one seeded permutation
    shard = shard_indices(nodes, rank, world, seed=0, epoch=0) + 2
    cu = lambda dct: {k: v.to(dev) for k, v in dct.items()}

    def stage(Bx, count, ctr0=0):
        out = []
        for i in range(count):
            tg = np.resize(shard[(i * Bx) % max(len(shard) - Bx, 1):], Bx) if len(shard) >= Bx else np.resize(shard, Bx)
            tgt, pair, num_pairs, labels = sampler.batch(tg, MODE_TRAIN, threads=threads, base_seed=rank, counter=ctr0 + i * Bx)
            out.append((cu(tgt), cu(pair), num_pairs.to(dev), labels.to(dev)))
        return out

    n_stage = min(args.steps + args.warmup, 8)
    staged = stage(B, n_stage)
    sampler_nodes_per_s = None
    if args.full:
        # sustained rate of the host sampler alone, as the live pipeline uses it: one warm call (worker pool and staging buffers
        # exist, pages touched), then back-to-back calls into one buffer
        slot = sampler.alloc(B, MODE_TRAIN)
        sampler.batch(np.resize(shard, B), MODE_TRAIN, out=slot, threads=threads, base_seed=rank, counter=n_stage * B)
        t0 = time.perf_counter()
        for i in range(4):
            sampler.batch(np.resize(shard[(i * B) % max(len(shard) - B, 1):], B), MODE_TRAIN, out=slot, threads=threads,
                          base_seed=rank, counter=(n_stage + 1 + i) * B)
        sampler_nodes_per_s = 4 * B / max(time.perf_counter() - t0, 1e-9)
        del slot

    def barrier():
        if exchange:
            dist.barrier()

    setup_s = time.perf_counter() - t_setup
    for i in range(args.warmup):
        trainer.train_step(staged[i % n_stage])
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    probe0 = clock_probe()
    t0 = time.perf_counter()
    loss_first = None
    for i in range(args.steps):
        l = trainer.train_step(staged[(args.warmup + i) % n_stage])
        if i == 0:
            loss_first = l.clone()  # device scalar of the first timed step (the engine recycles its output buffers); read after the timed region
    probe1 = clock_probe()
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if exchange:
        tt = torch.tensor([elapsed], device=dev, dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = tt.item()
    loss_last = trainer.last_loss.item()
    grad_norm_last = eng.grad_norm().item()
    if not (np.isfinite(loss_last) and np.isfinite(grad_norm_last)):
        # a step whose loss or pre-clip gradient norm is not finite does no learning (clip coefficient 0 / NaN parameters):
        # its time is not a measurement of the training step
        raise RuntimeError(f"bench: non-finite training state after the timed steps (loss {loss_last}, grad norm {grad_norm_last})")
    # (before any side measurement: those run more steps on the same engine)
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, last_step_outputs(trainer, eng))
    ms_per_step = elapsed / args.steps * 1e3
    value = world * B * args.steps / elapsed

    out = {
        "metric": "PMGT pre-train nodes/sec",
        "value": round(value, 2),
        "unit": "target nodes/s",
        "n_gpus": world,
        "steps": args.steps,
        "warmup": args.warmup,
        "ms_per_step": round(ms_per_step, 4),
        # shader clock the timed steps sustained (two probe launches around them: cycle counter vs the 100 MHz wall counter, per XCC)
        "sustained_sclk_mhz": sustained_sclk_mhz(probe0, probe1),
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": args.dtype,
        "data": ("synthetic (seeded circulant item graph with random offsets, N(0,1) visual/textual features drawn on the device, random-init weights)"
                 if big else "synthetic (seeded G(n,m)+ring item graph, N(0,1) visual/textual features, random-init weights)"),
        "config": {"workload": f"{args.workload}: {nodes} nodes / {edges} edges, L={L} H={H} d={d} I={I} S={S} "
                               f"(context=S tokens incl. target), B={B} targets/GPU/step, 12 sequences/target, "
                               f"dropout {args.dropout}, beta {args.beta:g}, clip 5.0, AdamW lr 1e-4 wd 1e-2",
                   "parallelism": f"dp{world}", "global_batch": world * B, "seq_len": S},
        "loss_first": round(loss_first.item(), 5),
        "loss_last": round(loss_last, 5),
        "grad_norm_last": round(grad_norm_last, 5),
        "setup_s": round(setup_s, 1),
        "side_stream_reductions": bool(args.overlap),
        "engine_options": list(args.engine_option),
        "allreduce": None,
    }
    if sampler_nodes_per_s is not None:
        # (per rank; vs_gpu_consumption < 1 means a run fed by the live sampler -- --end-to-end -- is bound by the host on this CPU share, not
        #  by the GPU: `value` is the pre-staged rate and does not depend on it)
        out["host_sampler"] = {"nodes_per_s": round(sampler_nodes_per_s, 1), "threads": threads, "cpus": os.cpu_count(),
                               "cpu_share": round(share, 1), "ranks_on_host": local_world,
                               "vs_gpu_consumption": round(sampler_nodes_per_s / max(value / world, 1e-9), 3)}
    if exchange:
        out["exchange_backend"] = dist.get_backend()
    if exchange and args.full:
        # (a side measurement: every rank enters it, and a failure inside it must not cost the line its headline numbers; a collective that
        #  raises does so on every rank at the same call, so the ranks stay in step)
        try:
            out["allreduce"] = measure_allreduce(trainer, eng, dev)
        except Exception as ex:      # noqa: BLE001
            out["allreduce"] = {"error": f"{type(ex).__name__}: {ex}"[:300]}

    flops_node = train_flops_per_node(d, I, L, S)
    out["train_gflop_per_node"] = round(flops_node / 1e9, 3)
    out["mfma_util_vs_bf16_dense_peak"] = round(value / world * flops_node / 1e12 / MFMA_BF16_PEAK_TFLOPS, 5)
    # north_star's target is quoted "on the PMGT encoder": the same rate priced on the encoder's algorithmic flops alone (SURVEY 8d:
    # "encoder 4.45" of the 5.38 GFLOP at C2 -- without the per-token feature projection and the NFR head)
    enc_node = encoder_flops_per_node(d, I, L, S)
    out["encoder_gflop_per_node"] = round(enc_node / 1e9, 3)
    out["mfma_util_encoder"] = round(value / world * enc_node / 1e12 / MFMA_BF16_PEAK_TFLOPS, 5)
    # the same rate priced on the flops the engine EXECUTES: table mode and the last-layer shortcut remove work the algorithmic
    # count above still includes (per-kernel matrix-pipe busy counters are under profiles/)
    dead = dead_branch_skipped(args, d, H, S)
    exec_node = executed_flops_per_node(d, I, L, S, nodes, B, dead_dot_branch=dead)
    out["executed_gflop_per_node"] = round(exec_node / 1e9, 3)
    out["mfma_util_executed"] = round(value / world * exec_node / 1e12 / MFMA_BF16_PEAK_TFLOPS, 5)
    if dead:
        # beta == 1: the engine skips the dead dot-product branch, so the full model's flop count prices work that is not done: the
        # utilisation keys carry the EXECUTED figure, the full-model ones stay under names that say so
        out["mfma_util_full_model_flops"] = out["mfma_util_vs_bf16_dense_peak"]
        out["mfma_util_encoder_full_model_flops"] = out["mfma_util_encoder"]
        out["mfma_util_vs_bf16_dense_peak"] = out["mfma_util_executed"]
        enc_exec = enc_node - 12 * S * 3 * L * (4 * d * d + 2 * S * d)
        out["mfma_util_encoder"] = round(value / world * enc_exec / 1e12 / MFMA_BF16_PEAK_TFLOPS, 5)
    if out["sustained_sclk_mhz"]:
        # the 2.5 PFLOP/s peak is quoted at 2.4 GHz; the timed steps ran at the clock above: the same utilisation against the peak at THAT clock
        out["mfma_util_encoder_at_sustained_clock"] = round(out["mfma_util_encoder"] * 2400.0 / out["sustained_sclk_mhz"], 5)

    # ---- per-phase HIP-event timers (separate pass, not part of `value`).  EVERY rank runs it, collectives included: the
    # control flow of all ranks is identical from init to destroy (only rank 0 prints), so no rank can be left alone in a
    # collective or tear the process group down while a peer still uses it.
    if args.full and not args.no_phase_profile:
        nprof = 5
        eng.profile_begin()
        for i in range(nprof):
            trainer.train_step(staged[i % n_stage])
        recs = eng.profile_records()
        seq = [n for n, _ in recs]
        # (launch order of the phases of one step: tools/make_traffic.py aligns the dispatches of a counter run with it)
        out["phase_sequence"] = seq[: len(seq) // nprof] if len(seq) % nprof == 0 else None
        # per phase: the MEDIAN launch (the last layer's dense blocks run on the compacted rows only: one launch in L is a fraction of the
        # others, and a mean over all of them would price a full launch's bytes / flops on less than a full launch's time)
        med_ms = {}
        for n, t in recs:
            med_ms.setdefault(n, []).append(t)
        med_ms = {n: float(np.median(v)) for n, v in med_ms.items()}
        prof = eng.profile_end()
        torch.cuda.synchronize()
        tot = sum(ms for _, ms in prof.values())
        phases = {k: {"launches_per_step": c // nprof, "ms_per_step": round(ms / nprof, 4), "share": round(ms / tot, 4),
                      "median_launch_ms": round(med_ms[k], 5)}
                  for k, (c, ms) in sorted(prof.items(), key=lambda kv: -kv[1][1])}
        out["phases"] = phases
        esz = 4 if args.dtype == "fp32" else 2
        M = 12 * B * S
        vc = dead_branch_skipped(args, d, H, S)
        dom = next((k for k in phases if phase_work(k, M, d, I, S, H, 1536, 768, B * (S - 1), esz, vc) is not None), next(iter(phases)))
        w = phase_work(dom, M, d, I, S, H, 1536, 768, B * (S - 1), esz, vc)
        avg_s = med_ms[dom] / 1e3
        if w is not None:
            flops, byts = w
            peak_t = MFMA_F32_PEAK_TFLOPS if args.dtype == "fp32" else MFMA_BF16_PEAK_TFLOPS
            if args.dtype == "fp8" and dom == "fwd.qkvc_attention":
                byts = M * d * (1 + 5 * esz) + M * 4        # x arrives as e4m3 rows + one fp32 scale per row; outputs stay bf16
            if flops > 0 and flops / (peak_t * 1e12) >= byts / (HBM_PEAK_GBS * 1e9):
                ach = flops / avg_s / 1e12
                out["roofline"] = {"kernel": dom, "bound": "mfma", "achieved": round(ach, 3), "peak": peak_t,
                                   "unit": "TFLOP/s", "frac": round(ach / peak_t, 5), "traffic": None,
                                   "avg_launch_ms": round(avg_s * 1e3, 5), "algorithmic_gflop_per_launch": round(flops / 1e9, 3)}
            else:
                ach = byts / avg_s / 1e9
                out["roofline"] = {"kernel": dom, "bound": "hbm", "achieved": round(ach, 2), "peak": HBM_PEAK_GBS,
                                   "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 5), "traffic": None,
                                   "avg_launch_ms": round(avg_s * 1e3, 5), "algorithmic_mb_per_launch": round(byts / 1e6, 3)}

        # the three most expensive phases that have an algorithmic model, each against the roof that bounds it (the step has several kernels
        # within 2x of each other: one line is not the picture)
        peak_t = MFMA_F32_PEAK_TFLOPS if args.dtype == "fp32" else MFMA_BF16_PEAK_TFLOPS
        top = []
        for k in phases:
            wk = phase_work(k, M, d, I, S, H, 1536, 768, B * (S - 1), esz, vc)
            if wk is None or len(top) == 3:
                continue
            c_k, ms_k = prof[k]
            t_k = med_ms[k] / 1e3
            fl, by = wk
            mf = fl > 0 and fl / (peak_t * 1e12) >= by / (HBM_PEAK_GBS * 1e9)
            ach = fl / t_k / 1e12 if mf else by / t_k / 1e9
            top.append({"kernel": k, "bound": "mfma" if mf else "hbm", "achieved": round(ach, 2), "unit": "TFLOP/s" if mf else "GB/s",
                        "frac": round(ach / (peak_t if mf else HBM_PEAK_GBS), 5), "avg_launch_ms": round(t_k * 1e3, 5),
                        "launches_per_step": c_k // nprof, "traffic": None, "traffic_ratio": None,
                        "algorithmic_mb_per_launch": round(by / 1e6, 3)})
        out["roofline_top3"] = top

    # HBM traffic of the dominant kernel: PMC counters cannot be read from inside this process (rocprofv3 collects them
    # in separate passes, tools/gpu_profile.sh); the committed summary of the last such run is quoted when it is for
    # this workload, else traffic stays null.
    if "roofline" in out:
        try:
            wl = traffic_key(args.workload, args.intermediate, args.beta, B)
            tname = "traffic.json" if wl == "c2" else f"traffic_{wl}.json"
            tr = json.load(open(os.path.join(ROOT, "profiles", tname)))
            fresh = tr.get("kernel_sources_sha") == kernel_sources_sha()       # measured on THESE kernels, else it is stale: null
            if fresh and tr.get("workload_key", tr["workload"]) == wl and tr["batch"] == B and args.dtype == "bf16":
                for ent in [out["roofline"]] + out.get("roofline_top3", []):
                    ph = tr["phases"].get(ent["kernel"])
                    if not ph:
                        continue
                    ent["traffic"] = ph["hbm_mb_per_launch"]
                    ent["traffic_src"] = "profiles/" + tname            # (MB per launch: 2 x FETCH_SIZE + WRITE_SIZE with the guide's gfx950 corrections)
                    ent["traffic_unit"] = "MB per launch (2 x FETCH_SIZE + WRITE_SIZE, " + tr["source"] + ")"
                    if "algorithmic_mb_per_launch" in ent:
                        ent["traffic_ratio"] = round(ph["hbm_mb_per_launch"] / ent["algorithmic_mb_per_launch"], 3)
                    if "matrix_pipe_busy" in ph:        # SQ_VALU_MFMA_BUSY_CYCLES / (4 x SQ_BUSY_CU_CYCLES) of the same profile set
                        ent["matrix_pipe_busy"] = ph["matrix_pipe_busy"]
                        ent["valu_per_mfma"] = ph.get("valu_per_mfma")
                out["step_hbm_gb"] = tr.get("step_hbm_gb")
        except (OSError, KeyError, ValueError):
            pass

    # ---- batch sizes of the reference's own entry points (N = 1): B=32 = scripts/run_pmgt.sh:11, B=256 = the CLI default
    # (train.py:33-38); eager launches and, where capture works, the whole step replayed as ONE hipGraph
    if world == 1 and args.full and not args.no_batch_sweep:
        sweep = {}
        for Bx in (32, 256):
            if Bx == B:
                continue
            st_x = stage(Bx, 4, ctr0=10 ** 6)
            # eager launches at these sizes are ~100 kernels of 5 - 30 us: a launch thread that shares its host with other tenants shows up
            # directly (one pass measured 2.3 ms where its neighbours measured 1.26), so: the best of three passes of 30 steps, all three reported
            runs = [time_steps(trainer, st_x, steps=30, warmup=5) * 1e3 for _ in range(3)]
            ms = min(runs)
            ent = {"nodes_per_s": round(Bx / ms * 1e3, 1), "ms_per_step": round(ms, 4), "ms_per_step_passes": [round(r, 4) for r in runs]}
            try:
                replay = trainer.capture_step(st_x[0])
                for _ in range(3):
                    replay()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(30):
                    replay()
                torch.cuda.synchronize()
                gms = (time.perf_counter() - t0) / 30 * 1e3
                ent["hipgraph_replay"] = {"nodes_per_s": round(Bx / gms * 1e3, 1), "ms_per_step": round(gms, 4)}
            except Exception as exc:                      # capture is an optimisation, never a reason to lose the bench line
                ent["hipgraph_replay"] = {"error": repr(exc)[:200]}
            sweep[str(Bx)] = ent
        # ... and above the headline's batch: the metric names no batch size, and a 288-GB device takes much larger shards (B = 4 096 is 1.57 M
        # tokens, ~52 GB of activations) -- the launches' fill / drain and the tile tails shrink with it (one box: 113.4k -> 117.6k -> 121.5k nodes/s)
        for Bx in (2048, 4096):
            if Bx <= B or args.workload not in ("c2", "c3"):
                continue
            try:
                st_x = stage(Bx, 3, ctr0=2 * 10 ** 6)
                ms = time_steps(trainer, st_x, steps=8, warmup=3) * 1e3
                sweep[str(Bx)] = {"nodes_per_s": round(Bx / ms * 1e3, 1), "ms_per_step": round(ms, 4)}
                del st_x
            except Exception as exc:                      # (memory, a 32-bit offset bound of a kernel ...): the headline does not depend on it
                sweep[str(Bx)] = {"error": repr(exc)[:200]}
        out["batch_sweep"] = sweep

    # ---- end to end with the live host sampler (threaded C++ MCNSampling -> pinned slots -> side-stream H2D): the rate a
    # training job sees; `value` above is the pre-staged rate the metric is defined on.  Every rank runs it (symmetric).
    # (at N > 1 only on request: the data-parallel numbers the driver collects are the pre-staged `value`; the multi-rank live pipeline
    # has only been rehearsed over gloo on one GPU)
    if args.full and not args.no_end_to_end and (world == 1 or args.end_to_end):
        # untimed pass first: pinned slots, device slots and the worker pool exist, pages touched, and (N = 1) the step is captured once
        # per slot -- the timed pass replays it with one launch per step (a launch thread that loses its CPU mid-step on a shared
        # host otherwise shows up as GPU idle time inside the step)
        live_graphs = world == 1 and not args.force_exchange
        trainer.run_live(sampler, shard, B, steps=6, threads=threads, graphs=live_graphs)
        e2e = trainer.run_live(sampler, shard, B, steps=max(min(args.steps, 40), 10), threads=threads, graphs=live_graphs)
        if world > 1:
            tt = torch.tensor([e2e["ms_per_step"]], device=dev, dtype=torch.float64)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            e2e["ms_per_step"] = round(tt.item(), 3)
            e2e["nodes_per_s"] = round(world * B / tt.item() * 1e3, 1)
        e2e["vs_prestaged"] = round(e2e["nodes_per_s"] / value, 4)
        out["end_to_end"] = e2e

    # ---- the other single-GPU configurations of BASELINE.json that are quoted anywhere: c4 shapes (10^6 nodes, L6 d512 S64) in bf16 and
    # in the fp8 mode (config 5), B = 256, ten steps each, in a child process of their own (a fresh engine and workspace; this
    # process only waits).  A child that does not deliver within the budget is reported as skipped with the reason.
    if rank == 0 and world == 1 and args.full and args.workload == "c2" and not args.no_extra_workloads:
        out["workloads"] = extra_workloads()

    # ---- CPU baseline: the oracle (CPU restatement pinned to the reference) on a bounded sample
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(cfg, graph, S, args.dropout)

    if rank == 0:
        detail_path = write_detail(out, args.detail_out)
        print("bench detail: " + json.dumps(out), file=sys.stderr)
        print(compact_line(out, detail_path), file=line_out)
        line_out.flush()
    if exchange:
        torch.cuda.synchronize()
        dist.barrier()                      # nobody tears the group down while a peer is still inside a collective
        dist.destroy_process_group()


# (BASELINE.json's configs 4 / 5 name the graph and the model, not a batch size: B = 256 is the reference's CLI default; the third line is the
#  same model with a shard sized for a 288-GB GPU -- 786 432 tokens per step -- where the d = 512 kernels' per-launch
#  fill / drain is a smaller share: +5 % nodes/s on one box)
EXTRA_WORKLOADS = (("c4_bf16", ["--workload", "c4", "--batch", "256", "--dtype", "bf16"]),
                   ("c5_fp8", ["--workload", "c4", "--batch", "256", "--dtype", "fp8"]),
                   ("c4_bf16_b1024", ["--workload", "c4", "--batch", "1024", "--dtype", "bf16", "--steps", "5", "--warmup", "2"]),
                   # SURVEY 8(d)'s I = 4 d rows (the author's own ratio: hidden 32 / intermediate 128, scripts/run_pmgt.sh:18): 9.00 and 100.6 GFLOP per node
                   ("c2_i1024", ["--workload", "c2", "--batch", "1024", "--dtype", "bf16", "--intermediate", "1024"]),
                   ("c4_i2048", ["--workload", "c4", "--batch", "256", "--dtype", "bf16", "--intermediate", "2048"]),
                   # the author's own attention mix (scripts/run_pmgt.sh:24: --beta 1.0): the dot-product branch is dead, the fused kernels project, store
                   # and differentiate V | C only; the flop count of the line stays the algorithmic one of the full model
                   ("c2_beta1", ["--workload", "c2", "--batch", "1024", "--dtype", "bf16", "--beta", "1.0"]))
EXTRA_BUDGET_S = 150.0


def extra_workloads():
    import subprocess
    import tempfile
    res = {}
    for name, extra in EXTRA_WORKLOADS:
        # (the child's stdout is its own compact line; the parent reads the child's full record from a file of its own)
        tmp = tempfile.NamedTemporaryFile(prefix=f"pmgt_bench_{name}_", suffix=".json", delete=False)
        tmp.close()
        cmd = [sys.executable, os.path.abspath(__file__), "--steps", "10", "--warmup", "3", "--full", "--no-cpu-baseline", "--no-end-to-end",
               "--no-batch-sweep", "--no-extra-workloads", "--detail-out", tmp.name] + extra
        t0 = time.perf_counter()
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=EXTRA_BUDGET_S)
            line = [ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
            if r.returncode != 0 or not line or os.path.getsize(tmp.name) == 0:
                res[name] = {"skipped": f"child exited with {r.returncode}: {r.stderr.strip()[-300:]}"}
                continue
            d = json.load(open(tmp.name))
            res[name] = {"nodes_per_s": d["value"], "ms_per_step": d["ms_per_step"], "batch": int(extra[extra.index("--batch") + 1]), "steps": d["steps"],
                         "train_gflop_per_node": d.get("train_gflop_per_node"),
                         "mfma_util_vs_bf16_dense_peak": d.get("mfma_util_vs_bf16_dense_peak"), "mfma_util_encoder": d.get("mfma_util_encoder"),
                         "mfma_util_executed": d.get("mfma_util_executed"), "roofline": d.get("roofline"), "roofline_top3": d.get("roofline_top3"),
                         "sustained_sclk_mhz": d.get("sustained_sclk_mhz"),
                         "loss_first": d.get("loss_first"), "loss_last": d.get("loss_last"), "setup_s": d.get("setup_s"),
                         "wall_s": round(time.perf_counter() - t0, 1),
                         "phases_top": dict(list(d.get("phases", {}).items())[:8])}
            if "fp8" in extra:
                res[name]["parity_mode_only"] = True
        except subprocess.TimeoutExpired:
            res[name] = {"skipped": f"graph build + staging + 13 steps did not finish within {EXTRA_BUDGET_S:.0f} s"}
        except Exception as exc:                      # an extra line is never a reason to lose the headline
            res[name] = {"skipped": repr(exc)[:300]}
        finally:
            try:
                os.unlink(tmp.name)
            except OSError:
                pass
    return res


# ---- the stdout line.  The driver keeps a bounded tail of stdout and parses the JSON line out of it: round 5's line had grown to 20 KB
# (six child workloads x (roofline + top-3 + phases) + the full phase map) and its head -- the headline keys -- was the part that got
# lost.  stdout now carries ONE line of at most LINE_BUDGET bytes; everything else goes to bench_detail.json (and stderr).
LINE_BUDGET = 4096
HEAD_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
             "config")
ROOF_KEYS = ("kernel", "bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_ratio", "traffic_src", "avg_launch_ms",
             "algorithmic_mb_per_launch", "algorithmic_gflop_per_launch", "matrix_pipe_busy")
SCALAR_KEYS = ("mfma_util_encoder", "mfma_util_vs_bf16_dense_peak", "mfma_util_executed", "mfma_util_encoder_at_sustained_clock",
               "sustained_sclk_mhz", "step_hbm_gb", "loss_first", "loss_last", "grad_norm_last", "exchange_backend")


def _pick(d, keys):
    return {k: d[k] for k in keys if isinstance(d, dict) and k in d}


def _compact_child(w):
    if not isinstance(w, dict) or "skipped" in w:
        return {"skipped": str((w or {}).get("skipped", "no record"))[:100]}
    c = _pick(w, ("nodes_per_s", "ms_per_step", "batch", "mfma_util_encoder", "mfma_util_executed"))
    r = w.get("roofline") or {}
    c.update({"roofline_kernel": r.get("kernel"), "roofline_frac": r.get("frac"), "traffic": r.get("traffic")})
    return c


def compact_line(out, detail_path=None, budget=LINE_BUDGET):
    """The ONE stdout line: the contract's keys first, then `roofline` and `cpu_baseline`, then short summaries of the side measurements, cut
    back (least important first) until the line is under `budget` bytes.  `out` is the full record that goes to the detail file."""
    c = _pick(out, HEAD_KEYS)
    if out.get("roofline"):
        c["roofline"] = _pick(out["roofline"], ROOF_KEYS)
    if out.get("cpu_baseline"):
        c["cpu_baseline"] = dict(out["cpu_baseline"])
        c["cpu_baseline"]["sample"] = str(c["cpu_baseline"].get("sample", ""))[:200]
    c.update(_pick(out, SCALAR_KEYS))
    optional = []       # (key, value) in the order they are given up when the line is too long: last entries go first
    if out.get("allreduce"):
        optional.append(("allreduce", _pick(out["allreduce"], ("buckets", "mb", "ms_per_step", "policy", "overlapped_with_backward", "error"))))
    if out.get("end_to_end"):
        optional.append(("end_to_end", _pick(out["end_to_end"], ("nodes_per_s", "ms_per_step", "vs_prestaged", "gpu_idle_ms_per_step"))))
    if out.get("workloads"):
        # (a child marked parity_mode_only -- the fp8 mode, measured at 0.98 - 0.99 of bf16: DESIGN section 3 -- stays in the detail file only)
        optional.append(("workloads", {k: _compact_child(v) for k, v in out["workloads"].items()
                                       if not (isinstance(v, dict) and v.get("parity_mode_only"))}))
    if out.get("host_sampler"):
        optional.append(("host_sampler", _pick(out["host_sampler"], ("nodes_per_s", "threads", "cpu_share", "vs_gpu_consumption"))))
    if out.get("batch_sweep"):
        optional.append(("batch_sweep", {k: (_pick(v, ("nodes_per_s", "ms_per_step")) or {"error": str(v.get("error", ""))[:60]})
                                         for k, v in out["batch_sweep"].items()}))
    if out.get("roofline_top3"):
        optional.append(("roofline_top3", [_pick(t, ("kernel", "bound", "frac", "avg_launch_ms", "traffic_ratio")) for t in out["roofline_top3"]]))
    if out.get("engine_options"):
        optional.append(("engine_options", out["engine_options"]))
    if detail_path:
        c["detail"] = os.path.basename(detail_path)
    for k, v in optional:
        c[k] = v
    line = json.dumps(c, separators=(",", ":"))
    while len(line.encode()) >= budget and optional:
        k, _ = optional.pop()
        c.pop(k, None)
        line = json.dumps(c, separators=(",", ":"))
    if len(line.encode()) >= budget:          # (cannot happen with the keys above; never print a line the driver cannot keep)
        c["config"] = {"workload": str(c.get("config", {}).get("workload", ""))[:120]}
        c.pop("cpu_baseline", None)
        line = json.dumps(c, separators=(",", ":"))
    return line


def write_detail(out, path=""):
    """Full record -> bench_detail.json next to this script (or `path`), plus a copy under gpurun_out/ when that directory exists (it is what
    travels back from a GPU box).  A read-only tree is not a reason to lose the line: returns the path written, or None."""
    written = None
    targets = [path] if path else [os.path.join(ROOT, "bench_detail.json")]
    if not path and os.path.isdir(os.path.join(ROOT, "gpurun_out")):
        targets.append(os.path.join(ROOT, "gpurun_out", "bench_detail.json"))
    for t in targets:
        try:
            with open(t, "w") as f:
                json.dump(out, f, indent=1)
            written = written or t
        except OSError:
            pass
    return written


def measure_allreduce(trainer, eng, dev):
    """The exchange step in numbers (every rank runs this; same collectives in the same order): the slices the trainer
    all-reduced in its last step, all-reduced again back to back on an otherwise idle GPU and timed with events on the stream
    they are ordered against -- the un-overlapped cost of one step's exchange (in the timed steps they run next to the
    backward pass of the earlier layers)."""
    import torch.distributed as dist
    ex = trainer._exchange
    sent = list(getattr(ex, "last_sent", [])) if ex is not None else [(0, eng.n_params)]
    if not sent:
        sent = [(0, eng.n_params)]
    scratch = torch.zeros_like(eng.grads)
    from pmgt_amd.parallel import backend_averages
    op = dist.ReduceOp.AVG if backend_averages(scratch.device) else dist.ReduceOp.SUM
    reps = 10
    for _ in range(2):
        for off, n in sent:
            dist.all_reduce(scratch[off: off + n], op=op)
    torch.cuda.synchronize()
    dist.barrier()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        works = [dist.all_reduce(scratch[off: off + n], op=op, async_op=True) for off, n in sent]
        for w in works:
            w.wait()
    e1.record()
    torch.cuda.synchronize()
    alone_ms = e0.elapsed_time(e1) / reps
    tt = torch.tensor([alone_ms], device=dev, dtype=torch.float64)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    return {"buckets": len(sent), "mb": round(sum(n for _, n in sent) * 4 / 1e6, 3), "ms_per_step": round(tt.item(), 4),
            "bucket_mb": [round(n * 4 / 1e6, 3) for _, n in sent], "policy": trainer.buckets,
            "overlapped_with_backward": ex is not None and trainer.buckets != "one",
            "note": "ms_per_step = the step's collectives issued back to back on an idle GPU (max over ranks); in the timed steps "
                    "they run next to the backward pass"}


def cpu_baseline(cfg, graph, S, dropout):
    """Times the CPU oracle (oracle/pmgt_oracle.py, checked against the reference's golden vectors) on the
    host cores: fp32, up to 16 threads, same shapes, B=8 targets per step (96 sequences), fwd+bwd+clip+AdamW."""
    from oracle import pmgt_oracle as po
    from pmgt_amd.datasets import MODE_TRAIN, MCNSampler
    cores = min(os.cpu_count() or 1, 16)     # more threads only slow these small ops down (oversubscription)
    torch.set_num_threads(cores)
    ocfg = po.default_cfg(hidden_size=cfg.hidden_size, num_hidden_layers=cfg.num_hidden_layers,
                          num_attention_heads=cfg.num_attention_heads, intermediate_size=cfg.intermediate_size,
                          hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout, beta=cfg.beta)
    n = graph.n_nodes
    params = po.synth_params(ocfg, 0)
    tables = po.synth_tables(n, ocfg["feat_hidden_sizes"], 0)
    Bc = 8
    smp = MCNSampler(graph, S - 1)
    batch = smp.batch(np.arange(2, 2 + Bc), MODE_TRAIN, threads=4, base_seed=1, counter=0)
    drop = (lambda x, site: torch.nn.functional.dropout(x, dropout, True)) if dropout > 0 else None
    state = {}
    times = []
    t_all = time.time()
    for it in range(12):
        t0 = time.perf_counter()
        p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        ids = batch[0]["node_ids"]
        r1, r2 = torch.rand(Bc, S - 1), torch.rand(Bc, S - 1)
        repl = torch.randint(2, n + 2, (Bc * (S - 1),))
        inj = po.nfr_masking(ids, n, r1, repl, r2)
        out = po.pretrain_forward(p, ocfg, tables, batch, training=True, nfr_inject=inj, drop=drop)
        out["loss"].backward()
        grads = {k: v.grad for k, v in p.items()}
        po.clip_grad_norm(grads, 5.0)
        po.adamw_step(params, grads, state, lr=1e-4, wd=1e-2)
        if it > 0:
            times.append(time.perf_counter() - t0)
        if time.time() - t_all > 20 and len(times) >= 2:
            break
    per = float(np.mean(times))
    return {"value": round(Bc / per, 2), "unit": "target nodes/s", "cores": cores, "kind": "port",
            "sample": f"{len(times)} timed steps of B={Bc} targets ({12 * Bc} sequences x S={S}) after 1 warm-up, "
                      f"fp32 torch CPU oracle, fwd+bwd+clip+AdamW, {per * 1e3:.0f} ms/step"}


if __name__ == "__main__":
    main()
