"""The device-side validation metrics, the parts that need no GPU: numpy restatements of the sort key and of the integer Mann-Whitney
formula of pmgt_amd/ops/eval_metrics.hip against roc_auc_score, the defaults of evaluate / fit, and the exported symbols."""
import inspect
import os
import subprocess

import numpy as np
import pytest


def key_of(scores):
    """eval_key() of pmgt_amd/ops/eval_metrics.h: -0.0 folded onto +0.0, negative values bit-flipped, the others with the sign bit set."""
    s = np.asarray(scores, dtype=np.float32)
    b = s.view(np.uint32).copy()
    b[s == 0] = 0
    neg = (b & np.uint32(0x80000000)) != 0
    return np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def two_u(labels, scores):
    """sum over tie groups of p (2 neg_below + q) on the keys, in Python integers; returns (twoU, n_pos, n_neg)."""
    keys = key_of(scores)
    lab = np.asarray(labels) != 0
    order = np.argsort(keys, kind="stable")
    k, l = keys[order], lab[order]
    starts = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])
    p = np.add.reduceat(l.astype(np.int64), starts)
    q = np.add.reduceat((~l).astype(np.int64), starts)
    neg_below = np.cumsum(q) - q
    return int(sum(int(a) * (2 * int(nb) + int(c)) for a, nb, c in zip(p, neg_below, q))), int(l.sum()), int((~l).sum())


def auc_from_integers(labels, scores):
    t, n_pos, n_neg = two_u(labels, scores)
    return float(t) / (2.0 * n_pos * n_neg)


def test_key_is_monotone_and_ties_the_two_zeros():
    rng = np.random.default_rng(0)
    tiny = np.float32(1e-45)
    special = np.array([-np.inf, np.inf, -0.0, 0.0, tiny, -tiny, 1e-39, -1e-39, np.finfo(np.float32).tiny, -np.finfo(np.float32).tiny,
                        np.finfo(np.float32).max, -np.finfo(np.float32).max, 1.0, -1.0], dtype=np.float32)
    bits = rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    s = np.concatenate([special, bits[~np.isnan(bits)], rng.standard_normal(2000).astype(np.float32)])
    s = np.sort(s)
    k = key_of(s).astype(np.int64)
    assert (np.diff(k) >= 0).all()
    assert ((np.diff(k) == 0) == (s[1:] == s[:-1])).all()        # equal keys exactly where the scores compare equal
    assert key_of([-0.0])[0] == key_of([0.0])[0] == 0x80000000
    assert key_of([-tiny])[0] < key_of([0.0])[0] < key_of([tiny])[0]
    assert key_of([np.inf])[0] == 0xFF800000 and key_of([-np.inf])[0] == 0x007FFFFF


@pytest.mark.parametrize("levels", [None, 4, 64, "zeros"])
def test_integer_formula_equals_roc_auc_score(levels):
    from pmgt_amd.trainer import roc_auc_score
    rng = np.random.default_rng(3)
    for n in (2, 3, 17, 256, 1000, 5000):
        s = rng.random(n).astype(np.float32)
        if levels == "zeros":
            s = np.where(rng.random(n) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
            s[rng.random(n) < 0.2] = np.float32(0.25)
        elif levels is not None:
            s = (np.floor(s * levels) / levels).astype(np.float32)
        lab = (rng.random(n) < 0.4).astype(np.float32)
        lab[0], lab[1] = 1.0, 0.0
        assert auc_from_integers(lab, s) == roc_auc_score(lab, s), (levels, n)


def test_host_metrics_stay_the_default():
    from pmgt_amd import trainer
    assert inspect.signature(trainer.evaluate).parameters["metrics"].default == "host"
    assert inspect.signature(trainer.fit).parameters["eval_metrics"].default == "host"
    with pytest.raises(ValueError):
        trainer.evaluate(None, None, np.arange(4), metrics="gpu")


def test_library_exports_the_eval_entries_and_no_rocprim_or_hipcub_symbol():
    from pmgt_amd import _build, _lib
    out = subprocess.run(["nm", "-D", _build.hip_lib_path()], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    for sym in ("pmgt_eval_workspace_bytes", "pmgt_eval_reset", "pmgt_eval_append", "pmgt_eval_reduce", "pmgt_op_eval_append_scores",
                "pmgt_op_eval_small_max"):
        assert sym in names, sym
        assert sym in _lib.HIP_SYMBOLS + _lib.OPS_SYMBOLS
    low = out.lower()
    assert "rocprim" not in low and "hipcub" not in low and "thrust" not in low
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pmgt_capi.h")).read()
    for sym in ("pmgt_eval_workspace_bytes", "pmgt_eval_reset", "pmgt_eval_append", "pmgt_eval_reduce"):
        decl = hdr[:hdr.index(sym + "(")]
        assert "pmgt/pmgt/trainer.py:162-195" in decl[decl.rindex("/*"):], sym      # every entry cites the interface it replaces
