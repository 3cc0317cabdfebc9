"""Pins the CPU oracle (oracle/) against golden vectors produced by the reference itself
(tests/golden/make_golden.py).  CPU-only."""
import hashlib

import numpy as np
import pytest
import torch

from oracle import pmgt_oracle as po
from oracle import sampler_oracle as so
from tests import golden_util as gu


# ----------------------------------------------------------------------------- sampler (G1, G7)
@pytest.mark.parametrize("gname", ["A", "B", "C"])
def test_sampler_oracle_bit_exact(gname):
    gold = gu.load("sampler_" + gname)
    n, edges, w = gu.graph(gname)
    assert np.array_equal(edges, gold["edges"]) and np.array_equal(w, gold["weights"])
    g = so.OrderedGraph(n, edges, w)
    idx = gold["idx"]
    for S in (6, 16, 32):
        for seed in (0, 1, 2):
            key = f"S{S}_seed{seed}_"
            np.random.seed(seed)
            ctx = [so.sample_context_neigh(g, t, [16, 8, 4], S - 1) for t in range(2, 10)]
            assert np.array_equal(np.array([c for c, _ in ctx]), gold[key + "ctx"])
            assert np.array_equal(np.array([k for _, k in ctx]), gold[key + "num_ctx"])
            for mode, kw in (("train_", {}), ("eval_", dict(is_training=False))):
                np.random.seed(seed)
                tgt, pair, num_pairs, labels = so.collate(
                    [so.dataset_getitem(g, int(i) + 2, S - 1, **kw) for i in idx])
                assert np.array_equal(tgt["node_ids"], gold[key + mode + "tgt_ids"])
                assert np.array_equal(tgt["attention_mask"], gold[key + mode + "tgt_mask"])
                assert np.array_equal(pair["node_ids"], gold[key + mode + "pair_ids"])
                assert np.array_equal(pair["attention_mask"], gold[key + mode + "pair_mask"])
                assert np.array_equal(num_pairs, gold[key + mode + "num_pairs"])
                assert np.array_equal(labels, gold[key + mode + "labels"])
            np.random.seed(seed)
            inf = so.collate([so.dataset_getitem(g, int(i) + 2, S - 1, is_inference=True) for i in idx])
            assert np.array_equal(inf["node_ids"], gold[key + "inf_ids"])
            assert np.array_equal(inf["attention_mask"], gold[key + "inf_mask"])


def test_split_oracle():
    gold = gu.load("split")
    for n, vs, seed in ((301, 0.2, 0), (7252, 0.2, 0), (10834, 0.1, 3)):
        tr, va = so.train_test_split_ids(n, vs, seed)
        k = f"n{n}_v{vs}_s{seed}_"
        assert list(gold[k + "sizes"]) == [len(tr), len(va)]
        assert np.array_equal(tr[:64], gold[k + "train_head"])
        assert hashlib.sha256(tr.astype(np.int64).tobytes()).digest() == gold[k + "train_sha"].tobytes()
        assert hashlib.sha256(va.astype(np.int64).tobytes()).digest() == gold[k + "valid_sha"].tobytes()


# ----------------------------------------------------------------------------- model (G2-G5)
@pytest.mark.parametrize("name", list(gu.MODEL_CASES))
def test_oracle_eval_forward(name):
    c = gu.model_case(name)
    gold, cfg, p, tabs = c["gold"], c["cfg"], c["params"], c["tables"]
    with torch.no_grad():
        out = po.pretrain_forward(p, cfg, tabs, c["batch"], training=False)
        np.testing.assert_allclose(out["loss"].item(), gold["eval_loss"], rtol=2e-6)
        np.testing.assert_allclose(out["logits"].numpy(), gold["eval_logits"], rtol=1e-5, atol=2e-6)
        tgt = c["batch"][0]
        h, hidden, probs = po.encoder_fwd(p, cfg, po.gather_feats(tgt["node_ids"], tabs),
                                          tgt["attention_mask"], want_probs=True, want_hidden=True)
        gu.check_stored(gold, "eval_last_hidden", h.numpy(), 1e-4, 2e-5)
        for i, hs in enumerate(hidden):
            gu.check_stored(gold, f"eval_hidden_{i}", hs.numpy(), 1e-4, 2e-5)
        for i, pr in enumerate(probs):
            gu.check_stored(gold, f"eval_attn_{i}", pr.numpy(), 1e-4, 1e-6)
        np.testing.assert_allclose(h[:, 0].numpy(), gold["inf_cls"], rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("name", list(gu.MODEL_CASES))
def test_oracle_train_loss_and_grads(name):
    c = gu.model_case(name)
    gold, cfg, tabs = c["gold"], c["cfg"], c["tables"]
    p = {k: v.clone().requires_grad_(True) for k, v in c["params"].items()}
    inj = gu.nfr_inject(gold, c["batch"][0]["node_ids"], c["n_nodes"])
    out = po.pretrain_forward(p, cfg, tabs, c["batch"], training=True, nfr_inject=inj)
    np.testing.assert_allclose(out["loss"].item(), gold["train_loss"], rtol=3e-6)
    np.testing.assert_allclose(out["logits"].detach().numpy(), gold["train_logits"], rtol=1e-5, atol=2e-6)
    out["loss"].backward()
    for k, v in p.items():
        gu.check_stored(gold, "grad/" + k, v.grad.numpy(), 2e-3, 2e-6)


@pytest.mark.parametrize("name", ["m1", "m1_pad", "m4"])
def test_oracle_optimizer_curve(name):
    """Several clip + AdamW steps.  The oracle runs in float64 from the fp32 parameters and tables the reference was loaded with: AdamW
    divides by sqrt(v), so a parameter whose gradient is the small remainder of terms that nearly cancel (a key bias) carries the rounding
    of that remainder into its value at ~lr per step.  In fp32 that rounding follows the summation order of the host's CPU kernels (thread
    count, vector width); in float64 it is negligible, and what is left to compare is the reference's own fp32 rounding in the fixture."""
    c = gu.model_case(name)
    gold, cfg = c["gold"], c["cfg"]
    tabs = [t.double() for t in c["tables"]]
    p = {k: v.double() for k, v in c["params"].items()}
    state = {}
    nsteps = len(gold["opt_losses"])
    for s in range(nsteps):
        pp = {k: v.clone().requires_grad_(True) for k, v in p.items()}
        inj = gu.nfr_inject(gold, c["batch"][0]["node_ids"], c["n_nodes"], prefix="opt_", suffix=f"_{s}")
        out = po.pretrain_forward(pp, cfg, tabs, c["batch"], training=True, nfr_inject=inj)
        if np.isnan(gold["opt_losses"][s]):      # reference quirk Q2: no masked token → NaN loss
            assert torch.isnan(out["loss"])
            return
        out["loss"].backward()
        grads = {k: v.grad for k, v in pp.items()}
        norm = po.clip_grad_norm(grads, 5.0)
        np.testing.assert_allclose(out["loss"].item(), gold["opt_losses"][s], rtol=2e-5)
        np.testing.assert_allclose(norm, gold["opt_gradnorms"][s], rtol=1e-4)
        po.adamw_step(p, grads, state, lr=1e-3, wd=1e-2)
    for k, v in p.items():
        gu.check_stored(gold, "final/" + k, v.numpy(), 1e-4, 1e-5)


@pytest.mark.parametrize("name", list(gu.NCF_CASES))
def test_ncf_second_caller_matches_reference(name):
    """PMGT_NCF (pmgt/pmgt_ncf/models.py) logits, BCE loss and every gradient — encoder and head — of the
    restatement equal the reference's; the frozen tables receive no gradient."""
    c = gu.ncf_case(name)
    gold = c["gold"]
    p = {k: v.clone().requires_grad_(True) for k, v in c["params"].items()}
    head = {k: v.clone().requires_grad_(True) for k, v in c["head"].items()}
    logits = po.ncf_forward(p, head, c["cfg"], c["tables"], c["user"], c["item"], c["num_layers"], c["model"])
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, c["labels"])
    loss.backward()
    np.testing.assert_allclose(logits.detach().numpy(), gold["logits"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(loss.item(), gold["loss"], rtol=1e-6)
    for k, v in list(p.items()) + list(head.items()):
        g = v.grad.numpy() if v.grad is not None else np.zeros(v.shape, np.float32)
        scale = float(np.sqrt((g.astype(np.float64) ** 2).mean())) + 1e-12
        gu.check_stored(gold, "grad/" + k, g, 2e-4, 2e-4 * scale + 1e-9)       # key.bias grads are exactly 0 in theory


@pytest.mark.parametrize("name,nsteps", [("curve_c", 8), ("curve_c2", 2)])
def test_loss_curve_over_fresh_batches_matches_reference(name, nsteps):
    """G9: the reference's sampler + model + clip + DenseSparseAdamW over fresh batches -- the toy configuration (30 steps) and
    the BENCHMARK configuration (curve_c2: 7 252-node graph, L4 H8 d256 S32, B = 32, lr 1e-4, 20 steps; north_star: "loss curve
    matching the reference within 1e-3").  The C++ sampler regenerates the batches from the seed; the oracle must reproduce
    the loss curve and gradient norms (CPU: the first steps only, to keep the suite short)."""
    c = gu.curve_case(name)
    gold = c["gold"]
    params = {k: v.clone() for k, v in c["params"].items()}
    state = {}
    for step, batch in gu.curve_batches(c):
        if step >= nsteps:
            break
        if step == 0:
            assert np.array_equal(batch[0]["node_ids"].numpy(), gold["tgt_ids_0"])
        p = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        inj = po.nfr_masking(batch[0]["node_ids"], c["n_nodes"], torch.from_numpy(gold[f"r1_{step}"]),
                             torch.from_numpy(gold[f"repl_{step}"]), torch.from_numpy(gold[f"r2_{step}"]))
        out = po.pretrain_forward(p, c["cfg"], c["tables"], batch, training=True, nfr_inject=inj)
        out["loss"].backward()
        grads = {k: v.grad for k, v in p.items()}
        norm = po.clip_grad_norm(grads, 5.0)
        po.adamw_step(params, grads, state, lr=c["lr"], wd=1e-2)
        np.testing.assert_allclose(out["loss"].item(), gold["losses"][step], rtol=3e-5)
        np.testing.assert_allclose(float(norm), gold["gradnorms"][step], rtol=3e-4)
