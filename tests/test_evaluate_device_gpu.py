"""evaluate(metrics="device") and fit(eval_metrics="device") against the host path on the world of tests/test_drivers_gpu.py (N = 300,
S = 16, d = 128, L = 2, fp32, valid split 0.3, batch 32 with a ragged last batch): identical loss/val, the AUC exact on the scores the
device stored and within 1e-6 of the host path's, the same training run around it, and two gloo ranks on one GPU."""
import json
import os
import socket
import time

import numpy as np
import pytest
import torch

from oracle import pmgt_oracle as po

pytestmark = pytest.mark.gpu

N, S = 300, 16
CFG = dict(hidden_size=128, num_hidden_layers=2, num_attention_heads=4, intermediate_size=128, hidden_dropout_prob=0.1,
           attention_probs_dropout_prob=0.1, beta=0.5)
BS, SEED, THREADS = 32, 17, 3


def make_world():
    from pmgt_amd.configuration_pmgt import PMGTConfig
    from pmgt_amd.datasets import MCNSampler, train_valid_split
    from pmgt_amd.engine import Engine
    from pmgt_amd.graph import synthetic_graph
    graph = synthetic_graph(N, 1500, seed=8)
    ocfg = po.default_cfg(**CFG)
    eng = Engine(PMGTConfig(**CFG), dtype="fp32", device="cuda:0", seed=0)
    eng.load_params(po.synth_params(ocfg, 12))
    eng.set_tables(*[t.numpy() for t in po.synth_tables(N, ocfg["feat_hidden_sizes"], 13)])
    train, valid = train_valid_split(N, 0.3, seed=4)
    return dict(eng=eng, smp=MCNSampler(graph, S - 1), train=train, valid=valid)


@pytest.fixture(scope="module")
def world():
    return make_world()


@pytest.fixture(scope="module")
def both(world):
    """The two paths on the same seed, computed once."""
    from pmgt_amd.trainer import evaluate
    args = dict(batch_size=BS, threads=THREADS, seed=SEED)
    assert len(world["valid"]) % BS != 0                      # ragged last batch
    return dict(host=evaluate(world["eng"], world["smp"], world["valid"], **args),
                device=evaluate(world["eng"], world["smp"], world["valid"], metrics="device", **args))


def test_loss_val_is_bit_identical_and_auc_within_the_driver_bound(both):
    print("host", both["host"], "device", both["device"])
    assert both["device"]["loss/val"] == both["host"]["loss/val"]
    assert abs(both["device"]["val/auc"] - both["host"]["val/auc"]) < 1e-6
    assert set(both["device"]) == set(both["host"]) and all(type(v) is float for v in both["device"].values())


def test_device_auc_is_roc_auc_score_of_the_scores_it_stored(world, both):
    from pmgt_amd.datasets import MODE_EVAL
    from pmgt_amd.metrics import ValidationMetrics
    from pmgt_amd.trainer import roc_auc_score
    valid, eng = world["valid"], world["eng"]
    vm = ValidationMetrics(eng.device, 2 * len(valid))
    labs = []
    for lo in range(0, len(valid), BS):
        tg = valid[lo: lo + BS]
        tgt, pair, num_pairs, labels = world["smp"].batch(tg, MODE_EVAL, threads=THREADS, base_seed=SEED, counter=lo)
        cu = lambda d: {k: v.to(eng.device) for k, v in d.items()}
        labels_dev = labels.to(eng.device)
        out = eng.pretrain_step((cu(tgt), cu(pair), num_pairs.to(eng.device), labels_dev), training=False, want_hidden=False)
        vm.update(out["logits"], labels_dev, out["loss"], len(tg))
        labs.append(labels.numpy().copy())
    got = vm.result()
    assert got == both["device"]
    assert vm.cursor == 2 * len(valid) and np.array_equal(vm.labels(), np.concatenate(labs))
    assert got["val/auc"] == roc_auc_score(vm.labels(), vm.scores())


def test_same_seed_same_dict(world, both):
    from pmgt_amd.trainer import evaluate
    args = dict(batch_size=BS, threads=THREADS, metrics="device")
    assert evaluate(world["eng"], world["smp"], world["valid"], seed=SEED, **args) == both["device"]
    assert evaluate(world["eng"], world["smp"], world["valid"], seed=SEED + 1, **args) != both["device"]


def test_fit_with_device_metrics_is_the_same_run(tmp_path):
    from pmgt_amd.trainer import Trainer, fit
    runs = {}
    for mode in ("host", "device"):
        w = make_world()
        tr = Trainer(w["eng"], lr=1e-3, weight_decay=1e-2, max_grad_norm=5.0)
        res = fit(tr, w["eng"], w["smp"], w["train"], w["valid"], batch_size=BS, max_epochs=2, early_criterion="auc", patience=5,
                  ckpt_dir=str(tmp_path / mode), seed=5, threads=2, valid_batch_size=BS, eval_metrics=mode)
        torch.cuda.synchronize()
        runs[mode] = dict(res=res, params=w["eng"].params.clone(), rng=w["eng"].rng_state.clone() if hasattr(w["eng"], "rng_state") else None)
    h, d = runs["host"]["res"], runs["device"]["res"]
    assert len(h["history"]) == len(d["history"]) == 2
    for a, b in zip(h["history"], d["history"]):
        assert a["loss/val"] == b["loss/val"] and a["epoch"] == b["epoch"]
        assert abs(a["val/auc"] - b["val/auc"]) < 1e-6
    best_epoch = lambda r: os.path.basename(r["best_model_path"]).split("-")[0]
    assert best_epoch(h) == best_epoch(d)
    assert torch.equal(runs["host"]["params"], runs["device"]["params"])       # validation touches neither the training state nor the RNG
    if runs["host"]["rng"] is not None:
        assert torch.equal(runs["host"]["rng"], runs["device"]["rng"])


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _eval_worker(rank, world_size, port, out_dir):
    import torch.distributed as dist
    from pmgt_amd.trainer import evaluate
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world_size)
    try:
        w = make_world()
        got = evaluate(w["eng"], w["smp"], w["valid"], batch_size=BS, threads=THREADS, seed=SEED, distributed=True, metrics="device")
        with open(os.path.join(out_dir, f"r{rank}.json"), "w") as f:
            json.dump({k: v.hex() for k, v in got.items()}, f)
    finally:
        dist.barrier()
        dist.destroy_process_group()


def test_two_gloo_ranks_report_the_single_process_result(tmp_path, both):
    import torch.multiprocessing as mp
    ctx = mp.spawn(_eval_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=False)
    deadline = time.monotonic() + 240                         # each rank under a time limit of its own
    try:
        while not ctx.join(timeout=2):
            assert time.monotonic() < deadline, "a rank did not finish in time"
    finally:
        for p in ctx.processes:
            if p.is_alive():
                p.kill()
    r0, r1 = ({k: float.fromhex(v) for k, v in json.load(open(tmp_path / f"r{r}.json")).items()} for r in range(2))
    assert r0 == r1
    np.testing.assert_allclose(r0["loss/val"], both["device"]["loss/val"], rtol=1e-12, atol=0)      # the summation order over ranks differs
    assert r0["val/auc"] == both["device"]["val/auc"]
