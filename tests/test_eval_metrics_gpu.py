"""Device-side validation metrics at the operator level, through the C ABI (pmgt_eval_* / pmgt_op_eval_* behind
pmgt_amd.metrics.ValidationMetrics): the AUC against roc_auc_score with `==`, error cases, loss accumulation, the sigmoid, determinism
and the absence of host syncs in update()."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# Distance between the stored fp32 score and the fp64 sigmoid of the same logit rounded to fp32, over SIGMOID_LOGITS.  By construction
# the score carries one rounding each of expf (ROCm documents 1 ULP), the add and the divide; on [-1, 1] the add halves expf's error, so
# the expected maximum is 1 ULP.  NOT YET MEASURED on the MI355X (the test prints the figure it finds); the bound is that expectation plus
# 1 ULP of headroom for another ROCm's expf, and stays below the 3 ULP above which a figure is a finding, not a bound.
SIGMOID_MEASURED_ULP = 1
SIGMOID_BOUND_ULP = SIGMOID_MEASURED_ULP + 1


def small_max():
    from pmgt_amd import _lib
    return int(_lib.hip().pmgt_op_eval_small_max())


def sizes():
    s = small_max()                      # the size switch = the element count of the one-workgroup path
    return [2, s - 1, s, s + 1, 70001]   # 70001: 34 tiles of 2048 and a ragged tail of 369


KINDS = ["continuous", "quant4", "all_equal", "signed_zeros", "negative_subnormal", "single_positive", "blocks"]


def make_case(kind, n, seed=0):
    rng = np.random.default_rng(seed + n)
    s = rng.random(n).astype(np.float32)
    lab = (rng.random(n) < 0.4).astype(np.float32)
    lab[0], lab[1] = 1.0, 0.0
    if kind == "quant4":                 # tie groups of ~n / 4: they straddle every tile boundary
        s = (np.floor(s * 4) / 4).astype(np.float32)
    elif kind == "all_equal":
        s[:] = 0.625
    elif kind == "signed_zeros":
        s = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        s[rng.random(n) < 0.2] = 0.25
    elif kind == "negative_subnormal":
        s = rng.standard_normal(n).astype(np.float32)
        sub = rng.integers(-40, 41, n).astype(np.float32) * np.float32(1e-45)       # +-subnormals, many ties, both zeros' neighbours
        pick = rng.random(n) < 0.5
        s[pick] = sub[pick]
        s[rng.random(n) < 0.05] = -np.finfo(np.float32).max      # the ends of the finite range (sklearn refuses infinities)
        s[rng.random(n) < 0.05] = np.finfo(np.float32).max
    elif kind == "single_positive":
        lab[:] = 0.0
        lab[int(rng.integers(0, n))] = 1.0
    elif kind == "blocks":
        lab[:] = 0.0
        lab[: max(n // 2, 1)] = 1.0
    return s, lab


def device_result(scores, labels, chunks=3, capacity=None):
    from pmgt_amd.metrics import ValidationMetrics
    n = len(scores)
    vm = ValidationMetrics(DEV, capacity or n)
    sd, ld = torch.from_numpy(scores).to(DEV), torch.from_numpy(labels).to(DEV)
    bounds = np.linspace(0, n, min(chunks, n) + 1).astype(int)
    for a, b in zip(bounds[:-1], bounds[1:]):
        vm.update_scores(sd[a:b], ld[a:b])
    return vm


@pytest.mark.parametrize("kind", KINDS)
def test_auc_equals_roc_auc_score_exactly(kind):
    from sklearn.metrics import roc_auc_score as sk
    from pmgt_amd.trainer import roc_auc_score
    for n in sizes():
        s, lab = make_case(kind, n)
        vm = device_result(s, lab)
        got = vm.result()["val/auc"]
        want = roc_auc_score(lab, s)
        print(f"{kind} n={n}: device {got!r} host {want!r}")
        assert got == want, (kind, n, got, want)
        assert abs(got - sk(lab, s.astype(np.float64))) < 1e-12, (kind, n)
        if kind == "all_equal":
            assert got == 0.5
        assert np.array_equal(vm.scores().view(np.uint32), s.view(np.uint32)) and np.array_equal(vm.labels(), lab)      # stored as given


def test_infinite_scores_sort_at_the_ends():
    """+-Inf are ordinary scores for the key function; roc_auc_score on the host accepts them (sklearn does not, so no comparison there)."""
    from pmgt_amd.trainer import roc_auc_score
    for n in (300, small_max() + 300):
        s, lab = make_case("negative_subnormal", n, seed=2)
        rng = np.random.default_rng(n)
        s[rng.random(n) < 0.1] = -np.inf
        s[rng.random(n) < 0.1] = np.inf
        assert device_result(s, lab).result()["val/auc"] == roc_auc_score(lab, s), n


def test_one_class_nan_and_capacity_errors_and_the_guard_region_stays_untouched():
    from pmgt_amd import _lib
    from pmgt_amd.metrics import ValidationMetrics
    lib = _lib.hip()
    s, lab = make_case("continuous", 300)
    for only in (0.0, 1.0):
        vm = device_result(s, np.full_like(lab, only))
        with pytest.raises(ValueError, match="Only one class present in y_true. ROC AUC score is not defined in that case."):
            vm.result()
    bad = s.copy()
    bad[[3, 77, 250]] = np.nan
    with pytest.raises(ValueError, match="3 of 300 scores are NaN"):
        device_result(bad, lab).result()
    logits = torch.from_numpy(s).to(DEV)
    logits[5] = float("nan")                                 # through the sigmoid entry too
    vm = ValidationMetrics(DEV, 300)
    vm.update(logits, torch.from_numpy(lab).to(DEV))
    with pytest.raises(ValueError, match="1 of 300 scores are NaN"):
        vm.result()
    # a workspace followed by a guard region: appends up to the last slot and a reduce on either path leave it alone, an append past the
    # capacity is refused by the Python cursor AND by the C entry (-2), and writes nothing
    for cap in (300, small_max() + 905):
        nbytes, guard = ValidationMetrics.workspace_bytes(cap), 8192
        buf = torch.full((nbytes + guard,), 0xA5, dtype=torch.uint8, device=DEV)
        vm = ValidationMetrics(DEV, cap, workspace=buf)
        s, lab = make_case("quant4", cap)
        sd, ld = torch.from_numpy(s).to(DEV), torch.from_numpy(lab).to(DEV)
        vm.update_scores(sd[: cap - 7], ld[: cap - 7])
        with pytest.raises(ValueError, match="do not fit the capacity"):
            vm.update_scores(sd[:8], ld[:8])
        with pytest.raises(ValueError, match="do not fit the capacity"):
            vm.update(sd[:1], ld[:1], offset=cap)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        assert lib.pmgt_op_eval_append_scores(buf.data_ptr(), cap, sd.data_ptr(), ld.data_ptr(), 0, cap - 7, 8, 0, stream) == -2
        assert lib.pmgt_eval_append(buf.data_ptr(), cap, sd.data_ptr(), ld.data_ptr(), 0, cap, 1, 0, stream) == -2
        assert lib.pmgt_eval_reduce(buf.data_ptr(), cap, cap + 1, stream) == -2
        vm.update_scores(sd[cap - 7:], ld[cap - 7:])         # exactly full
        from pmgt_amd.trainer import roc_auc_score
        assert vm.result()["val/auc"] == roc_auc_score(lab, s)
        torch.cuda.synchronize()
        assert bool((buf[nbytes:] == 0xA5).all()), cap


def test_loss_accumulates_as_the_host_loop_does():
    from pmgt_amd.metrics import ValidationMetrics
    rng = np.random.default_rng(5)
    losses = (rng.random(9) * 3).astype(np.float32)
    counts = [32, 32, 7, 256, 1, 100, 32, 13, 29]
    s, lab = make_case("continuous", 2 * sum(counts))
    vm = ValidationMetrics(DEV, len(s))
    ld, sd, labd = torch.from_numpy(losses).to(DEV), torch.from_numpy(s).to(DEV), torch.from_numpy(lab).to(DEV)
    lo, loss_sum = 0, 0.0
    for i, c in enumerate(counts):
        vm.update(sd[lo: lo + 2 * c], labd[lo: lo + 2 * c], ld[i], c)
        lo += 2 * c
        loss_sum += float(losses[i]) * c
    assert vm.result()["loss/val"] == float(loss_sum / sum(counts))
    assert vm.loss_sum() == loss_sum


SIGMOID_LOGITS = np.concatenate([np.linspace(-1.0, 1.0, 8193), [20, -20, 88, -88, 104, -104]]).astype(np.float32)


def ordered(x):
    b = np.asarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


def test_sigmoid_against_the_fp64_sigmoid():
    from pmgt_amd.metrics import ValidationMetrics
    x = SIGMOID_LOGITS
    vm = ValidationMetrics(DEV, len(x))
    vm.update(torch.from_numpy(x).to(DEV), torch.zeros(len(x), device=DEV))
    got = vm.scores()
    with np.errstate(over="ignore"):
        want = (1.0 / (1.0 + np.exp(-x.astype(np.float64)))).astype(np.float32)
    ulp = np.abs(ordered(got) - ordered(want))
    worst = int(ulp.argmax())
    print(f"sigmoid: max ULP distance {int(ulp.max())} at logit {x[worst]!r} (device {got[worst]!r}, fp64 -> fp32 {want[worst]!r}); "
          f"tail logits {x[-6:].tolist()} -> {got[-6:].tolist()} vs {want[-6:].tolist()}")
    assert int(ulp.max()) <= SIGMOID_BOUND_ULP


@pytest.mark.parametrize("n", [3000, 70001])
def test_reduce_is_deterministic_and_independent_of_the_update_order(n):
    from pmgt_amd.metrics import ValidationMetrics
    s, lab = make_case("quant4", n, seed=9)
    sd, ld = torch.from_numpy(s).to(DEV), torch.from_numpy(lab).to(DEV)
    bounds = np.linspace(0, n, 8).astype(int)
    pieces = list(zip(bounds[:-1], bounds[1:]))
    vm = ValidationMetrics(DEV, n)
    for a, b in pieces:
        vm.update_scores(sd[a:b], ld[a:b], offset=int(a))
    first = vm.statistic()
    assert vm.statistic() == first                           # the same workspace, reduced again
    vm.reset()
    for i in np.random.default_rng(1).permutation(len(pieces)):
        a, b = pieces[i]
        vm.update_scores(sd[a:b], ld[a:b], offset=int(a))
    again = vm.statistic()
    assert (again["twoU"], again["n_pos"], again["n_neg"]) == (first["twoU"], first["n_pos"], first["n_neg"])
    from tests.test_eval_metrics_cpu import two_u
    assert (first["twoU"], first["n_pos"], first["n_neg"]) == two_u(lab, s)


def test_update_never_syncs():
    from pmgt_amd.metrics import ValidationMetrics
    s, lab = make_case("continuous", 5000)
    sd, ld, loss = torch.from_numpy(s).to(DEV), torch.from_numpy(lab).to(DEV), torch.ones(1, device=DEV)
    vm = ValidationMetrics(DEV, 5000)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        vm.reset()
        for lo in range(0, 5000, 500):
            vm.update(sd[lo: lo + 500], ld[lo: lo + 500], loss[0], 250)
    finally:
        torch.cuda.set_sync_debug_mode(before)
    r = vm.result()
    assert r["loss/val"] == 1.0 and 0.0 < r["val/auc"] < 1.0
