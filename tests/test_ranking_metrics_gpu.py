"""Device-side ranking metrics at the operator level (pmgt_rank_* behind pmgt_amd.metrics.RankingMetrics, kernels in
pmgt_amd/ops/ranking_metrics.hip): per-user nDCG@k / Recall@k `==` the host path over row lengths around every boundary of the kernel (the
wave, the workgroup, the row limit), score kinds with ties, the reference's fixture, ragged rows, refused arguments, determinism, the loss
bound and the absence of host syncs in update()."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ROW_LENGTHS = [1, 2, 63, 64, 65, 100, 255, 256, 257, 1000, 4096]
USERS = [1, 3, 257]
KINDS = ["continuous", "quant4", "all_equal", "signed_zeros", "inf_ends"]
KS = [(1,), (10, 20), (1, 7, 64, 1024)]


def make_scores(kind, U, Cn, rng):
    s = (rng.standard_normal((U, Cn)) * 2).astype(np.float32)
    if kind == "quant4":                     # four levels: tie groups of ~C / 4
        s = (np.floor(rng.random((U, Cn)) * 4) / 4).astype(np.float32)
    elif kind == "all_equal":
        s[:] = 0.625
    elif kind == "signed_zeros":
        s = np.where(rng.random((U, Cn)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        s[rng.random((U, Cn)) < 0.2] = 0.25
    elif kind == "inf_ends":
        s[rng.random((U, Cn)) < 0.1] = -np.inf
        s[rng.random((U, Cn)) < 0.1] = np.inf
    return s


def make_labels(U, Cn, max_k, rng, first_mode=0):
    """Positives at random positions; the rows cycle through n_pos = 1, C and (just) above max(ks)."""
    lab = np.zeros((U, Cn), dtype=np.float32)
    for r in range(U):
        n_pos = (1, Cn, min(Cn, max_k + 5))[(r + first_mode) % 3]
        lab[r, rng.choice(Cn, size=n_pos, replace=False)] = 1.0
    return lab


def device_metrics(scores, labels, counts=None, ks=(10, 20), **kw):
    from pmgt_amd.metrics import RankingMetrics
    rm = RankingMetrics(DEV, len(scores), ks, **kw)
    rm.update(torch.from_numpy(scores).to(DEV), torch.from_numpy(labels).to(DEV),
              None if counts is None else torch.from_numpy(np.asarray(counts, dtype=np.int32)).to(DEV))
    return rm


def assert_same_ranking(got, want, ks, what):
    for k in ks:
        assert np.array_equal(got["ndcg"][k], want["ndcg"][k]), (what, k, "ndcg")
        assert np.array_equal(got["recall"][k], want["recall"][k]), (what, k, "recall")
    assert np.array_equal(got["n_pos"], want["n_pos"]) and np.array_equal(got["nan"], want["nan"]), what
    assert np.array_equal(got["empty"], want["empty"]), what


@pytest.mark.parametrize("Cn", ROW_LENGTHS)
def test_per_user_metrics_equal_the_host_path(Cn):
    """Every score kind and every set of cut-offs at this row length; the number of users cycles so that, over the row lengths, every
    (users, kind, cut-offs) combination runs; within a batch the rows cycle through the three n_pos cases."""
    from pmgt_amd.evaluation import ranking_metrics_host
    rng = np.random.default_rng(Cn)
    ci = ROW_LENGTHS.index(Cn)
    seen = set()
    for a, kind in enumerate(KINDS):
        for b, ks in enumerate(KS):
            U = USERS[(a + b + ci) % 3]
            seen.add(U)
            s = make_scores(kind, U, Cn, rng)
            lab = make_labels(U, Cn, ks[-1], rng, first_mode=a + b)
            got = device_metrics(s, lab, ks=ks).per_user()
            want = ranking_metrics_host(s, lab, None, ks)
            assert_same_ranking(got, want, ks, (kind, ks, U, Cn))
            assert not got["nan"].any() and not got["empty"].any()
    assert seen == set(USERS)


@pytest.mark.parametrize("name", ["ranking_metrics_64x128", "ranking_metrics_5x1000"])
def test_the_reference_fixture_per_user(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    rm = device_metrics(g["logits"], g["labels"])
    got = rm.per_user()
    U = len(g["logits"])
    for k in (10, 20):
        assert np.array_equal(got["ndcg"][k], g[f"n{k}_user"]) and np.array_equal(got["recall"][k], g[f"r{k}_user"]), k
    res = rm.result()
    for key in ("n10", "n20", "r10", "r20"):
        print(f"{name} {key}: device {res[key]!r} reference {float(g[key])!r}")
        assert abs(res[key] - float(g[key])) <= U * 2.0 ** -52, key


def test_ragged_rows_never_read_their_padding():
    from pmgt_amd.evaluation import ranking_metrics_host
    rng = np.random.default_rng(7)
    U, Cn, ks = 37, 300, (10, 20)
    s = make_scores("quant4", U, Cn, rng)
    lab = make_labels(U, Cn, 20, rng)
    counts = rng.integers(1, Cn + 1, U).astype(np.int32)
    counts[:3] = (1, Cn, 64)
    lab[np.arange(U), rng.integers(0, counts)] = 1.0             # a positive among the live candidates of every row
    live = np.arange(Cn)[None, :] < counts[:, None]
    clean = device_metrics(np.where(live, s, np.float32(0)), np.where(live, lab, np.float32(0)), counts, ks)
    dirty_s, dirty_l = np.where(live, s, np.float32(np.nan)), np.where(live, lab, np.float32(1))      # NaN scores, positive labels in the padding
    dirty = device_metrics(dirty_s, dirty_l, counts, ks)
    a, b = clean.per_user(), dirty.per_user()
    assert_same_ranking(b, a, ks, "padding")
    assert np.array_equal(a["loss"].view(np.uint32), b["loss"].view(np.uint32))
    assert_same_ranking(b, ranking_metrics_host(dirty_s, dirty_l, counts, ks), ks, "host")
    st = dirty.statistic()
    assert st["n_nan"] == 0 and st["n_empty"] == 0 and st["n_users"] == U
    assert dirty.result() == clean.result()


def test_a_live_nan_and_an_empty_row_make_result_raise():
    rng = np.random.default_rng(8)
    s = make_scores("continuous", 9, 70, rng)
    lab = make_labels(9, 70, 20, rng)
    bad = s.copy()
    bad[2, 69] = np.nan
    bad[5, 0] = np.nan
    rm = device_metrics(bad, lab)
    with pytest.raises(ValueError, match="2 of 9 users have a NaN logit"):
        rm.result()
    assert rm.per_user()["nan"].tolist() == [False, False, True, False, False, True, False, False, False]
    none = lab.copy()
    none[4] = 0.0
    rm = device_metrics(s, none)
    with pytest.raises(ValueError, match="1 of 9 users have no positive candidate"):
        rm.result()
    pu = rm.per_user()
    assert pu["empty"].tolist() == [r == 4 for r in range(9)] and pu["n_pos"][4] == 0 and pu["ndcg"][10][4] == 0.0 and pu["recall"][20][4] == 0.0
    # a positive in the padding only is no positive
    counts = np.full(9, 70, np.int32)
    counts[4] = 30
    none[4, 50] = 1.0
    with pytest.raises(ValueError, match="1 of 9 users have no positive candidate"):
        device_metrics(s, none, counts).result()


def test_a_label_other_than_one_is_a_positive_and_counts_as_one_in_the_loss():
    from pmgt_amd.evaluation import ranking_metrics_host
    rng = np.random.default_rng(13)
    s = make_scores("continuous", 5, 300, rng)
    lab = make_labels(5, 300, 20, rng)
    odd = np.where(lab != 0, rng.choice(np.array([2.0, -1.0, 0.5, 1e-30, np.inf], np.float32), size=lab.shape), np.float32(0)).astype(np.float32)
    a, b = device_metrics(s, lab).per_user(), device_metrics(s, odd).per_user()
    assert_same_ranking(b, a, (10, 20), "labels")
    assert np.array_equal(a["loss"].view(np.uint32), b["loss"].view(np.uint32))
    host = ranking_metrics_host(s, odd, None, (10, 20))
    assert_same_ranking(b, host, (10, 20), "host")
    assert np.abs(b["loss"].astype(np.float64) - host["loss"]).max() <= (300 + 8) * 2.0 ** -24 * host["loss"].max()


def test_slots_no_update_reached_are_counted_and_refused():
    from pmgt_amd.metrics import RankingMetrics
    rng = np.random.default_rng(14)
    s, lab = make_scores("continuous", 10, 40, rng), make_labels(10, 40, 20, rng)
    sd, ld = torch.from_numpy(s).to(DEV), torch.from_numpy(lab).to(DEV)
    rm = RankingMetrics(DEV, 10)
    rm.update(sd[:3], ld[:3], offset=0)
    rm.update(sd[6:], ld[6:], offset=6)                       # slots 3, 4, 5 stay as reset left them
    assert rm.statistic()["n_unwritten"] == 3
    with pytest.raises(ValueError, match="3 of the 10 user slots below the cursor were never written"):
        rm.result()
    pu = rm.per_user()
    assert pu["unwritten"].tolist() == [3 <= r < 6 for r in range(10)] and not pu["ndcg"][10][3:6].any() and not pu["loss"][3:6].any()
    rm.update(sd[3:6], ld[3:6], offset=3)
    full = device_metrics(s, lab)
    assert rm.result() == full.result() and rm.statistic()["n_unwritten"] == 0
    rm.reset()                                                # a reset marks them all again
    rm.update(sd[:1], ld[:1], offset=9)
    assert rm.statistic()["n_unwritten"] == 9


def test_refused_arguments_write_nothing_and_the_guard_region_stays_untouched():
    from pmgt_amd import _lib
    from pmgt_amd.metrics import RankingMetrics, discount_tables
    lib = _lib.hip()
    rng = np.random.default_rng(9)
    U, Cn, ks = 70, 130, (10, 20)           # 70 users: the records are rounded up to 128 slots
    nbytes, guard = RankingMetrics.workspace_bytes(U, len(ks)), 8192
    buf = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device=DEV)
    rm = RankingMetrics(DEV, U, ks, workspace=buf)
    s, lab = make_scores("continuous", U, Cn, rng), make_labels(U, Cn, 20, rng)
    sd, ld = torch.from_numpy(s).to(DEV), torch.from_numpy(lab).to(DEV)
    cd = torch.full((U,), Cn, dtype=torch.int32, device=DEV)
    rm.update(sd[:40], ld[:40], cd[:40])
    torch.cuda.synchronize()
    before = buf.clone()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ws, x, y, c = buf.data_ptr(), sd.data_ptr(), ld.data_ptr(), cd.data_ptr()
    disc, idcg = discount_tables(1024)
    ints = lambda *v: (C.c_int * len(v))(*v)
    refused = [
        lib.pmgt_rank_append(ws, U, x, y, c, Cn, 40, 31, stream),            # slots past max_users
        lib.pmgt_rank_append(ws, U, x, y, c, Cn, U, 1, stream),
        lib.pmgt_rank_append(ws, U, x, y, c, Cn, -1, 1, stream),
        lib.pmgt_rank_append(ws, U, x, y, c, Cn, 2 ** 63 - 1, 2 ** 63 - 1, stream),      # a sum that would wrap round
        lib.pmgt_rank_append(ws, U, x, y, c, Cn, 1, 2 ** 63 - 1, stream),
        lib.pmgt_rank_append(ws, U, x, y, c, Cn, 2 ** 63 - 1, 1, stream),
        lib.pmgt_rank_append(ws, U, x, y, c, 0, 0, 1, stream),               # row_stride outside [1, 4096]
        lib.pmgt_rank_append(ws, U, x, y, c, 4097, 0, 1, stream),
        lib.pmgt_rank_append(ws, U, 0, y, c, Cn, 0, 1, stream),              # NULL
        lib.pmgt_rank_append(ws, U, x, 0, c, Cn, 0, 1, stream),
        lib.pmgt_rank_append(0, U, x, y, c, Cn, 0, 1, stream),
        lib.pmgt_rank_append(ws + 8, U, x, y, c, Cn, 0, 1, stream),          # misaligned
        lib.pmgt_rank_append(ws, U, x + 2, y, c, Cn, 0, 1, stream),
        lib.pmgt_rank_append(ws, U, x, y, c + 1, Cn, 0, 1, stream),
        lib.pmgt_rank_append(ws, 0, x, y, c, Cn, 0, 1, stream),
        lib.pmgt_rank_reduce(ws, U, U + 1, stream),
        lib.pmgt_rank_reduce(ws, U, 0, stream),
        lib.pmgt_rank_reduce(ws + 4, U, 1, stream),
        lib.pmgt_rank_reset(ws, U, ints(20, 10), 2, disc.ctypes.data, idcg.ctypes.data, stream),         # not strictly increasing
        lib.pmgt_rank_reset(ws, U, ints(10, 10), 2, disc.ctypes.data, idcg.ctypes.data, stream),
        lib.pmgt_rank_reset(ws, U, ints(0, 10), 2, disc.ctypes.data, idcg.ctypes.data, stream),          # outside [1, 1024]
        lib.pmgt_rank_reset(ws, U, ints(10, 1025), 2, disc.ctypes.data, idcg.ctypes.data, stream),
        lib.pmgt_rank_reset(ws, U, ints(1, 2, 3, 4, 5), 5, disc.ctypes.data, idcg.ctypes.data, stream),  # more than 4
        lib.pmgt_rank_reset(ws, U, ints(10, 20), 0, disc.ctypes.data, idcg.ctypes.data, stream),
        lib.pmgt_rank_reset(ws, U, 0, 2, disc.ctypes.data, idcg.ctypes.data, stream),
        lib.pmgt_rank_reset(ws, U, ints(10, 20), 2, 0, idcg.ctypes.data, stream),
        lib.pmgt_rank_reset(ws, U, ints(10, 20), 2, disc.ctypes.data + 4, idcg.ctypes.data, stream),
        lib.pmgt_rank_reset(0, U, ints(10, 20), 2, disc.ctypes.data, idcg.ctypes.data, stream),
    ]
    assert refused == [-2] * len(refused), refused
    assert lib.pmgt_rank_workspace_bytes(0, 2) < 0 and lib.pmgt_rank_workspace_bytes(U, 0) < 0 and lib.pmgt_rank_workspace_bytes(U, 5) < 0
    # a workspace reset for another max_users: the launch runs and writes nothing
    assert lib.pmgt_rank_append(ws, U - 1, x, y, c, Cn, 0, 1, stream) == 0
    assert lib.pmgt_rank_reduce(ws, U - 1, 1, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    with pytest.raises(ValueError, match="do not fit max_users"):
        rm.update(sd[:31], ld[:31], cd[:31])
    with pytest.raises(ValueError, match="do not fit max_users"):
        rm.update(sd[:1], ld[:1], offset=U)
    with pytest.raises(ValueError, match="outside"):
        rm.update(torch.zeros(1, 4097, device=DEV), torch.zeros(1, 4097, device=DEV))
    rm.update(sd[40:], ld[40:], cd[40:])       # exactly full, up to the last slot
    from pmgt_amd.evaluation import ranking_metrics_host
    assert_same_ranking(rm.per_user(), ranking_metrics_host(s, lab, None, ks), ks, "full")
    rm.result()
    torch.cuda.synchronize()
    assert bool((buf[nbytes:] == 0xA5).all())


def test_the_result_does_not_depend_on_how_the_users_were_split_and_repeats_bitwise():
    from pmgt_amd.evaluation import ranking_metrics_host, summarize_ranking
    from pmgt_amd.metrics import RankingMetrics
    rng = np.random.default_rng(10)
    U, Cn, ks = 1300, 200, (5, 10, 20)
    s = make_scores("quant4", U, Cn, rng) + (rng.random((U, Cn)) < 0.5).astype(np.float32)
    lab = make_labels(U, Cn, 20, rng)
    sd, ld = torch.from_numpy(s).to(DEV), torch.from_numpy(lab).to(DEV)
    nbytes = RankingMetrics.workspace_bytes(U, len(ks))

    def run(pieces):
        rm = RankingMetrics(DEV, U, ks, workspace=torch.zeros(nbytes, dtype=torch.uint8, device=DEV))
        for a, b in pieces:
            rm.update(sd[a:b], ld[a:b], offset=a)
        st = rm.statistic()
        return rm, st, rm._ws.cpu().numpy().copy()

    one, st_one, raw_one = run([(0, U)])
    _, st_three, raw_three = run([(911, U), (257, 911), (0, 257)])           # three updates, reversed order, arbitrary offsets
    _, st_again, raw_again = run([(0, U)])
    assert st_one == st_three == st_again
    assert np.array_equal(raw_one, raw_three) and np.array_equal(raw_one, raw_again)      # header and records, bit for bit
    assert one.statistic() == st_one                                                     # the same workspace, reduced again
    host = ranking_metrics_host(s, lab, None, ks)
    want, got = summarize_ranking(host, ks), one.result()
    for k in ks:
        for key in (f"n{k}", f"r{k}"):
            print(f"{key}: device {got[key]!r} host {want[key]!r}")
            assert abs(got[key] - want[key]) <= U * 2.0 ** -52, key


def test_per_user_loss_against_the_fp64_formula():
    """max(x, 0) - x y + log1p(exp(-|x|)), mean over the live candidates.  The terms are non-negative, so any fp32 summation order stays
    within (C - 1) u of the exact sum, plus a few ULP per term from expf / log1pf: the bound is (C + 8) * 2^-24, relative."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for Cn in (1, 65, 257, 1000, 4096):
        U = 33
        x = (rng.standard_normal((U, Cn)) * 4).astype(np.float32)
        x[0, : min(Cn, 8)] = np.array([0.0, -0.0, 88.0, -88.0, 104.0, -104.0, 1e-30, 20.0], np.float32)[:Cn]
        lab = (rng.random((U, Cn)) < 0.3).astype(np.float32)
        lab[:, 0] = 1.0
        counts = rng.integers(1, Cn + 1, U).astype(np.int32)
        counts[0] = Cn
        got = device_metrics(x, lab, counts).per_user()["loss"].astype(np.float64)
        xd = x.astype(np.float64)
        term = np.maximum(xd, 0.0) - xd * lab + np.log1p(np.exp(-np.abs(xd)))
        live = np.arange(Cn)[None, :] < counts[:, None]
        want = np.where(live, term, 0.0).sum(axis=1) / counts
        rel = np.abs(got - want) / want
        print(f"C={Cn}: largest relative loss error {rel.max():.3e} (bound {(Cn + 8) * 2.0 ** -24:.3e})")
        worst = max(worst, float(rel.max() / ((Cn + 8) * 2.0 ** -24)))
        assert rel.max() <= (Cn + 8) * 2.0 ** -24, Cn
    print(f"largest share of the bound used: {worst:.3f}")


def test_update_never_syncs():
    from pmgt_amd.metrics import RankingMetrics
    rng = np.random.default_rng(12)
    U, Cn = 600, 128
    s, lab = make_scores("continuous", U, Cn, rng), make_labels(U, Cn, 20, rng)
    sd, ld = torch.from_numpy(s).to(DEV), torch.from_numpy(lab).to(DEV)
    cd = torch.full((U,), Cn, dtype=torch.int32, device=DEV)
    rm = RankingMetrics(DEV, U)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        rm.reset()
        for lo in range(0, U, 100):
            rm.update(sd[lo: lo + 100], ld[lo: lo + 100], cd[lo: lo + 100] if lo % 200 else None)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    r = rm.result()
    assert set(r) == {"n10", "n20", "r10", "r20", "loss"} and 0.0 < r["n10"] <= 1.0 and 0.0 < r["r20"] <= 1.0 and r["loss"] > 0.0
