"""In-tree build of the native libraries (gfx950 only).

  pmgt_amd/lib/libpmgt_hip.so      HIP kernels + engine + C ABI   (hipcc --offload-arch=gfx950)
  pmgt_amd/lib/libpmgt_sampler.so  host MCNSampling               (g++)

hipcc cross-compiles without a GPU, so this runs in the dev container; the built .so files travel
to the GPU box with the repo snapshot (they are git-ignored, not gpurun-ignored).
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "lib")
OBJ = os.path.join(HERE, "csrc", "_obj")
# outside csrc/ (bench.py fingerprints the kernel sources there): the host-only single-kernel entries of the test surface
# (include/pmgt_ops.h), the learning-rate-scheduled and the guarded form of the optimizer step, and the device-side validation metrics, none of
# which the measured step launches; the weight-averaging kernels (SWA / EMA update, content swap) and the ranking metrics (nDCG@k / Recall@k
# per user row) for the same reason; likewise the fused NCF scoring of users against the whole catalogue and the per-row top-k selection;
# the compacted-row test entries of the last-layer shortcut (host code around the engine's own kernels); the forward, backward and
# gradient kernels that train the NCF head over a frozen item table (what the two NCF sources share is ops/ncf_head.h, tracked with the headers);
# the forward and the gradients of the Deep & Cross Network of the click-through experiment; the CLS gather / scatter between the encoder and a
# head that is fine-tuned with it; the gradient kernels of the reference's stand-alone NCF class (LayerNorm layers, kind GMF) and the fused
# scoring of that class against the whole catalogue; the fused scoring of the Deep & Cross Network against the whole catalogue (the deep tower on
# the NCF scoring tile, the collapsed cross net in its epilogue), out of csrc/ for ncf_score.hip's reason; the exact whole-catalogue ranks of
# held-out items and the metrics from them, out of csrc/ for ranking_metrics.hip's reason; the fused clip + SGD step of the pair trainers
# (the reference's --optim sgd), out of csrc/ for optimizer_step.hip's reason (what the two share is ops/optimizer_step.h);
# the several-buffer step of the fine-tune trainer under a schedule, the guard or SGD (segments_step.hip), which shares that header too;
# the co-review counts that build the item graph from interactions (item_graph.hip), a preprocessing stage the step never launches;
# the item-by-item dot / cosine scores from the encoder's embedding table (item_sim.hip), out of csrc/ for ncf_score.hip's reason;
# the item-kNN scores of users from their histories over that table (history_score.hip: item_sim.hip's tile with a segmented reduction), likewise;
# the truncated, weighted item-kNN scores over a precomputed neighbour index (knn_score.hip: gather, LDS accumulators, store), likewise
OPS_SOURCES = [os.path.join(HERE, "ops", "row_ops.hip"), os.path.join(HERE, "ops", "optimizer_step.hip"),
               os.path.join(HERE, "ops", "dropout_keep.hip"), os.path.join(HERE, "ops", "eval_metrics.hip"),
               os.path.join(HERE, "ops", "weight_average.hip"), os.path.join(HERE, "ops", "ranking_metrics.hip"),
               os.path.join(HERE, "ops", "ncf_score.hip"), os.path.join(HERE, "ops", "topk_rows.hip"),
               os.path.join(HERE, "ops", "compact_rows.hip"), os.path.join(HERE, "ops", "ncf_train.hip"),
               os.path.join(HERE, "ops", "dcn_train.hip"), os.path.join(HERE, "ops", "cls_ops.hip"),
               os.path.join(HERE, "ops", "ncf_model_train.hip"), os.path.join(HERE, "ops", "ncf_model_score.hip"),
               os.path.join(HERE, "ops", "dcn_score.hip"), os.path.join(HERE, "ops", "catalogue_rank.hip"),
               os.path.join(HERE, "ops", "sgd_step.hip"), os.path.join(HERE, "ops", "segments_step.hip"),
               os.path.join(HERE, "ops", "item_graph.hip"), os.path.join(HERE, "ops", "item_sim.hip"),
               os.path.join(HERE, "ops", "history_score.hip"), os.path.join(HERE, "ops", "knn_score.hip")]
HIP_SOURCES = ["gemm.hip", "gemm_ws.hip", "gemm_wsr.hip", "gemm_rowln.hip", "fp8.hip", "rowops.hip", "attention.hip", "attention_mfma.hip", "qkvc_attn.hip", "segsum.hip", "loss.hip", "optim.hip", "engine.hip"]
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
# -amdgpu-mfma-vgpr-form: MFMA accumulators stay in architectural VGPRs (no v_accvgpr_read moves before every VALU
# use of a result: -7 % VALU instructions in the attention backward, which is VALU-issue-bound)
# -fno-slp-vectorize: the SLP vectoriser pairs adjacent fp32 adds / multiplies of the epilogues into v_pk_add_f32 / v_pk_mul_f32,
# which issue no faster than the two scalar instructions they replace on gfx950 and cost v_mov shuffles to build the register
# pairs (streaming-GEMM LayerNorm epilogue: 485 -> 287 packed + move instructions per tile); the epilogues are VALU-bound:
# LayerNorm backward 1.09 -> 0.97 ms per step, step 11.00 -> 10.84 ms
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-fno-slp-vectorize", "-mllvm", "-amdgpu-mfma-vgpr-form=1"] + os.environ.get("PMGT_EXTRA_HIP_FLAGS", "").split()


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("build failed: %s\n%s\n%s" % (" ".join(cmd), r.stdout, r.stderr))


def hip_lib_path():
    return os.path.join(LIB, "libpmgt_hip.so")


def sampler_lib_path():
    return os.path.join(LIB, "libpmgt_sampler.so")


def build_hip(force=False):
    os.makedirs(LIB, exist_ok=True)
    os.makedirs(OBJ, exist_ok=True)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers += [os.path.join(os.path.dirname(HERE), "include", h) for h in ("pmgt_capi.h", "pmgt_ops.h")]
    headers += [os.path.join(HERE, "ops", f) for f in os.listdir(os.path.join(HERE, "ops")) if f.endswith(".h")]
    jobs, objs = [], []
    for src in [os.path.join(CSRC, s) for s in HIP_SOURCES] + OPS_SOURCES:
        obj = os.path.join(OBJ, os.path.basename(src).replace(".hip", ".o"))
        objs.append(obj)
        if force or _newer(obj, [src] + headers):
            jobs.append([HIPCC] + HIP_FLAGS + ["-c", src, "-o", obj])
    with ThreadPoolExecutor(max_workers=6) as ex:
        list(ex.map(_run, jobs))
    out = hip_lib_path()
    if force or jobs or _newer(out, objs):
        _run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out] + objs)
    return out


def build_sampler(force=False):
    os.makedirs(LIB, exist_ok=True)
    src = os.path.join(CSRC, "sampler.cpp")
    out = sampler_lib_path()
    hdr = os.path.join(os.path.dirname(HERE), "include", "pmgt_capi.h")
    if force or _newer(out, [src, hdr]):
        _run(["g++", "-O3", "-std=c++17", "-fPIC", "-shared", "-pthread", "-o", out, src])
    return out


def build_all(force=False):
    return build_hip(force), build_sampler(force)


if __name__ == "__main__":
    print(build_all(force="--force" in sys.argv))
