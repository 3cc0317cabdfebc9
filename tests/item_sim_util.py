"""Shared by the tests of pmgt_item_sim_score: the sizes, the seeded tables, the query lists, the planted table and the measure.

THE MEASURE is tests/test_ncf_score_gpu.py's, per case (n queries x I items; a pair's score reads its two rows alone, so every case is a
block of ONE host evaluation at the largest size), o64 / r32 = item_sim_host in fp64 / fp32:
    max|x - o64| <= C max(max|r32 - o64|, 2^-22 max|o64|),   C = 4.
A dot product of two random rows may cancel, so a table can be drawn on which a RIGHT fp32 realisation in another order of sums misses that
bound in some small case.  Such a table judges the order of a sum, not a kernel.  SEEDS therefore holds, per d, the first seed from 29 on
at which a SECOND fp32 realisation (second_realisation: a strictly sequential, UNFUSED ascending-k chain, every product and every sum
rounded -- worse than the kernel's fmaf chain --, the same for the squared norms; all numpy) keeps within C on every case of both metrics.
That is decided on the CPU by the yardstick's realisations alone (python -m tests.item_sim_util prints the search);
tests/test_item_sim_cpu.py asserts it."""
import functools

import numpy as np

from pmgt_amd.similar import METRICS, item_sim_host

ITEMS, DS, NS = (1, 31, 33, 127, 129, 300), (1, 8, 33, 100, 256, 1024), (1, 5, 67, 130)
EXACT_DS = (1, 8, 33, 64)                                    # the exact case: small integers, every sum exact in fp32
EPS = 1e-12
C_BOUND = 4.0
FIRST_SEED = 29
# the first seed from FIRST_SEED on at which second_realisation keeps within C_BOUND on every case (python -m tests.item_sim_util)
SEEDS = {d: 29 for d in DS}


def normal_table(d, seed):
    return np.random.default_rng(seed).standard_normal((ITEMS[-1], d)).astype(np.float32)


def integer_table(d, n_items=ITEMS[-1], seed=5):
    """entries in {-2 .. 2}: every product and every partial sum of up to 64 of them is exact in fp32, whatever the order"""
    return np.random.default_rng(seed).integers(-2, 3, size=(n_items, d)).astype(np.float32)


def queries_of(n_items):
    """NS[-1] query ids in [0, n_items), unordered, one id twice"""
    q = np.random.default_rng(7 + n_items).integers(0, n_items, size=NS[-1]).astype(np.int64)
    q[3] = q[0]
    return q


def second_realisation(table, metric, eps=EPS):
    """every item against every item in fp32 numpy in ANOTHER REALISATION: acc = acc + a_k * b_k one k after the other, product and sum
    each rounded to fp32; the squared norms the same way -> [I, I]"""
    f32 = np.float32
    t = np.asarray(table, dtype=f32)
    n_items, d = t.shape
    dot = np.zeros((n_items, n_items), dtype=f32)
    sq = np.zeros(n_items, dtype=f32)
    for k in range(d):
        col = t[:, k]
        dot = dot + col[:, None] * col[None, :]
        sq = sq + col * col
    assert dot.dtype == f32 and sq.dtype == f32
    if metric == "dot":
        return dot
    inv = (f32(1) / np.maximum(np.sqrt(sq), f32(eps))).astype(f32)
    j = np.arange(n_items)
    lo, hi = np.minimum(j[:, None], j[None, :]), np.maximum(j[:, None], j[None, :])
    return (dot * inv[lo]) * inv[hi]


def case_ratio(x, o64, r32, q, n_items):
    """max|x - o64| / max(max|r32 - o64|, 2^-22 max|o64|) for x [len(q), n_items] = the scores of the queries q against the first n_items items"""
    ref = o64[q][:, :n_items]
    floor = max(np.abs(r32[q][:, :n_items] - ref).max(), 2.0 ** -22 * np.abs(ref).max())
    return float(np.abs(np.asarray(x, dtype=np.float64) - ref).max() / floor)


def yardsticks(table, metric, eps=EPS):
    o64 = item_sim_host(table, None, metric, eps, np.float64)
    r32 = item_sim_host(table, None, metric, eps, np.float32)
    assert o64.dtype == np.float64 and r32.dtype == np.float32
    return o64, r32.astype(np.float64)


def second_worst(d, seed):
    """the largest ratio of second_realisation over the cases and both metrics on the table of `seed`"""
    table = normal_table(d, seed)
    worst = 0.0
    for metric in METRICS:
        o64, r32 = yardsticks(table, metric)
        x = second_realisation(table, metric)
        for n_items in ITEMS:
            q = queries_of(n_items)
            for n in NS:
                worst = max(worst, case_ratio(x[q[:n]][:, :n_items], o64, r32, q[:n], n_items))
    return worst


@functools.lru_cache(maxsize=None)
def world(d):
    """The table of SEEDS[d] and the two yardsticks of both metrics at the largest size; computed once, shared, never written"""
    table = normal_table(d, SEEDS[d])
    out = dict(table=table)
    for metric in METRICS:
        out[metric] = yardsticks(table, metric)
        for a in out[metric]:
            a.setflags(write=False)
    table.setflags(write=False)
    return out


PLANTED_ITEMS, PLANTED_CLUSTERS, PLANTED_SIZE = 40, 8, 5


@functools.lru_cache(maxsize=None)
def planted_table():
    """40 items in 8 clusters of 5: one-hot cluster centres plus small seeded noise, fp32 [40, 8]"""
    rng = np.random.default_rng(13)
    t = np.repeat(np.eye(PLANTED_CLUSTERS), PLANTED_SIZE, axis=0) + 0.05 * rng.standard_normal((PLANTED_ITEMS, PLANTED_CLUSTERS))
    t = t.astype(np.float32)
    t.setflags(write=False)
    return t


def planted_edges():
    """two held-out edges inside every cluster"""
    return np.array([(PLANTED_SIZE * c + a, PLANTED_SIZE * c + b) for c in range(PLANTED_CLUSTERS) for a, b in ((0, 1), (2, 4))], dtype=np.int64)


if __name__ == "__main__":                                   # the choice of SEEDS
    found = {}
    for d in DS:
        for seed in range(FIRST_SEED, FIRST_SEED + 200):
            worst = second_worst(d, seed)
            print("d", d, "seed", seed, f"the second realisation: largest ratio {worst:.2f}")
            if worst <= C_BOUND:
                found[d] = seed
                break
    print("SEEDS =", found)
