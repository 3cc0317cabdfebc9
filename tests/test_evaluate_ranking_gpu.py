"""evaluate_ranking end to end on the two PMGT_NCF golden cases (tests/golden_util.py: small graphs, hidden 64 / 128, golden weights):
the device path against the host path, PMGT_NCF.forward still at its golden logits after the head was factored out, and the loop without
a host sync."""
import numpy as np
import pytest
import torch

from tests import golden_util as gu

pytestmark = pytest.mark.gpu

KS = (10, 20)
NUM_NG = {"ncf_mlp": 50, "ncf_neumf": 100}


def build(name):
    from pmgt_amd.configuration_pmgt import PMGTConfig
    from pmgt_amd.datasets import MCNSampler, ranking_candidates
    from pmgt_amd.graph import CSRGraph
    from pmgt_amd.pmgt_ncf import PMGT_NCF
    c = gu.ncf_case(name)
    model = PMGT_NCF(user_num=c["users"], item_num=c["n_nodes"], factor_num=c["factor"], num_layers=c["num_layers"],
                     model=c["model"], config=PMGTConfig(**c["cfg"]), dtype="fp32")
    sd = model.state_dict()
    with torch.no_grad():
        for k, v in list(c["params"].items()) + list(c["head"].items()):
            sd[k].copy_(v)
    model.set_features([t.numpy() for t in c["tables"]])
    gname, S = gu.NCF_CASES[name][0], gu.NCF_CASES[name][2]
    n, edges, w = gu.graph(gname)
    sampler = MCNSampler(CSRGraph.from_edge_list(n, edges, w), max_ctx_neigh=S - 1)
    # a synthetic interaction list over the case's users and items: 1 .. 24 items per user, one user above max(ks)
    rng = np.random.default_rng(5)
    pairs = [(u, int(i)) for u in range(c["users"]) for i in rng.choice(n, size=24 if u == 2 else int(rng.integers(1, 9)), replace=False)]
    cands = ranking_candidates(pairs, c["users"], n, NUM_NG[name], seed=3)
    return dict(case=c, model=model, sampler=sampler, cands=cands)


@pytest.fixture(scope="module", params=["ncf_mlp", "ncf_neumf"])
def world(request):
    return build(request.param)


def test_device_path_equals_host_path(world):
    from pmgt_amd.trainer import evaluate_ranking
    model, sampler, cands = world["model"], world["sampler"], world["cands"]
    model.train()
    host, pu_h = evaluate_ranking(model, sampler, *cands, ks=KS, batch_users=4, metrics="host", per_user=True)
    dev, pu_d = evaluate_ranking(model, sampler, *cands, ks=KS, batch_users=4, metrics="device", per_user=True)
    assert model.training                                    # the mode the caller had is restored
    U, Cn = cands[1].shape
    assert set(host) == set(dev) == {"n10", "n20", "r10", "r20", "loss"}
    for k in KS:                                             # both rank the same logits
        assert np.array_equal(pu_d["ndcg"][k], pu_h["ndcg"][k]) and np.array_equal(pu_d["recall"][k], pu_h["recall"][k]), k
    assert np.array_equal(pu_d["n_pos"], pu_h["n_pos"]) and np.array_equal(pu_d["n_pos"], (cands[2] != 0).sum(axis=1))
    assert int(pu_d["n_pos"].max()) > max(KS)
    # the two may differ in the per-user loss, by (C + 8) * 2^-24 relative, and in the means, by the summation order of U values in [0, 1]
    rel = np.abs(pu_d["loss"].astype(np.float64) - pu_h["loss"].astype(np.float64)) / pu_h["loss"].astype(np.float64)
    print(f"largest relative loss distance device / host: {rel.max():.3e}")
    assert rel.max() <= (Cn + 8) * 2.0 ** -24
    for key in ("n10", "n20", "r10", "r20"):
        print(f"{key}: device {dev[key]!r} host {host[key]!r}")
        assert abs(dev[key] - host[key]) <= U * 2.0 ** -52, key
        assert 0.0 <= dev[key] <= 1.0
    print(f"loss: device {dev['loss']!r} host {host['loss']!r}")
    assert abs(dev["loss"] - host["loss"]) <= (Cn + 8) * 2.0 ** -24 * host["loss"]
    # the same call again: the same dict
    assert evaluate_ranking(model, sampler, *cands, ks=KS, batch_users=4, metrics="device") == dev
    # another split of the users over the batches changes nothing per user
    _, pu_b = evaluate_ranking(model, sampler, *cands, ks=KS, batch_users=256, metrics="device", per_user=True)
    for k in KS:
        assert np.array_equal(pu_b["recall"][k], pu_d["recall"][k]), k


def test_ids_outside_the_models_tables_are_refused_on_the_host(world):
    from pmgt_amd.trainer import evaluate_ranking
    model, sampler = world["model"], world["sampler"]
    users, cand, labels, counts = world["cands"]
    for bad_users, bad_cand, bad_counts, what in ((np.where(users == users[0], model.user_num, users), cand, counts, "users"),
                                                  (np.where(users == users[0], -1, users), cand, counts, "users"),
                                                  (users, np.where(cand == cand[0, 0], model.item_num, cand), counts, "candidates"),
                                                  (users, np.where(cand == cand[0, 0], -1, cand), counts, "candidates"),
                                                  (users, cand, np.where(counts == counts[0], cand.shape[1] + 1, counts), "counts"),
                                                  (users, cand, np.where(counts == counts[0], 0, counts), "counts")):
        for metrics in ("host", "device"):
            with pytest.raises(ValueError, match=what):
                evaluate_ranking(model, sampler, bad_users, bad_cand, labels, bad_counts, ks=KS, metrics=metrics)


def test_forward_still_equals_the_golden_logits(world):
    """PMGT_NCF.forward after the head moved into a method of its own: what test_ncf_second_caller_on_hip_encoder checks of the logits and
    the loss, in both modes."""
    c, model = world["case"], world["model"]
    gold = c["gold"]
    model.train()
    logits = model(c["user"], c["item"])
    loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, c["labels"].cuda())
    np.testing.assert_allclose(logits.detach().cpu().numpy(), gold["logits"], rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(loss.item(), gold["loss"], rtol=1e-4)
    model.eval()
    with torch.no_grad():
        np.testing.assert_allclose(model(c["user"], c["item"]).cpu().numpy(), gold["logits"], rtol=1e-4, atol=1e-5)
        # the head on the encoder's own CLS states is the forward
        dev = model.engine.device
        ids = c["item"]["node_ids"].to(dev)
        emb = model.bert.encode_ids(ids, attention_mask=c["item"]["attention_mask"].to(dev))[0][:, 0]
        assert torch.equal(model.head(c["user"].to(dev), ids[:, 0] - 2, emb), model(c["user"], c["item"]))


def test_the_loop_never_syncs(world):
    from pmgt_amd.metrics import RankingMetrics
    from pmgt_amd.trainer import encode_catalogue, evaluate_ranking, rank_users
    model, sampler, cands = world["model"], world["sampler"], world["cands"]
    dev = model.engine.device
    model.eval()
    table = encode_catalogue(model, sampler)
    assert table.dtype == torch.float32 and tuple(table.shape) == (world["case"]["n_nodes"], model.config.hidden_size) and table.device == dev
    on_dev = [torch.from_numpy(a).to(dev) for a in cands]
    rm = RankingMetrics(dev, len(cands[0]), KS)
    rank_users(model, table, *on_dev, sink=rm.update, batch_users=4)       # warm: the first call of a GEMM shape may load code
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rm.reset()
        rank_users(model, table, *on_dev, sink=rm.update, batch_users=4)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    assert rm.result() == evaluate_ranking(model, sampler, *cands, ks=KS, batch_users=4, metrics="device")
