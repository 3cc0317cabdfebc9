"""Shared by the tests of pmgt_dcn_score: the heads, the sizes, the seeded models and the measure.

THE MEASURE is tests/ncf_model_score_util.py's, per case (n users x I items, a block of one host evaluation at the largest size: a pair's
logit does not depend on the other pairs), o64 / r32 = dcn_scores_host in fp64 / fp32:
    max|x - o64| <= C max(max|r32 - o64|, 2^-22 max|o64|),   C = 4.
A LayerNorm divides by the spread of its row, the cross recurrence multiplies C factors and a logit is a sum that may cancel, so a model can
be drawn on which a RIGHT fp32 realisation in another order of sums misses that bound in some small case.  Such a model judges the order of
a sum, not a kernel.  SEEDS therefore holds, per head, the first seed from 29 on at which a SECOND fp32 realisation keeps within C on every
case: second_realisation is the COLLAPSED form the kernel computes (pmgt_amd/dcn_head.py's header: the cross net as one scalar per user row
plus one per item row), layer 0 of the deep net split into the per-user and the per-item product, every later product and the output dot
summed in reversed column order; all fp32 numpy.  That is decided on the CPU by the yardstick's realisations alone
(python -m tests.dcn_score_util prints the search); tests/test_dcn_score_cpu.py asserts it."""
import functools

import numpy as np

from pmgt_amd.dcn_head import ITEM_KEY, OUT_B, OUT_W, USER_KEY, _ln, dcn_row_scalars_host, dcn_score_constants, dcn_scores_host
from tests.dcn_util import random_dcn

# (factor_num, deep layers, cross layers, LayerNorm): the VALU path without and with LayerNorm (the second is scripts/run_dcn.sh's shape);
# E = 32, one block; E = 64 without LayerNorm; E = 256 over three layers; E = 256 over four; E = 256 with the last width 128 (four blocks
# in the output dot) and 9 row scalars; the VALU path at its widest, 128 features, and C = 6 without LayerNorm
HEADS = [(8, 1, 1, False), (16, 1, 4, True), (8, 2, 3, True), (16, 2, 2, False), (32, 3, 3, True), (16, 4, 2, True), (64, 2, 6, True),
         (64, 1, 6, False)]
NS, ITEMS = (1, 5, 67), (1, 31, 33, 65, 300)
USER_NUM = 80
EPS = 1e-12
C_BOUND = 4.0
FIRST_SEED = 29
# the first seed from FIRST_SEED on at which second_realisation keeps within C_BOUND on every case (python -m tests.dcn_score_util)
SEEDS = {h: 29 for h in HEADS}
# the head that is scored again with another layer_norm_eps, in kernel and yardstick: a dropped eps misses
EPS_HEAD, EPS_OTHER = (8, 2, 3, True), 0.5


def head_id(h):
    return f"f{h[0]}-L{h[1]}-C{h[2]}-{'ln' if h[3] else 'noln'}"


def users_of():
    users = np.random.default_rng(7).integers(0, USER_NUM, size=NS[-1])
    users[3] = users[0]                                      # a user twice
    return users


def model_weights(head, seed, user_num=USER_NUM, item_num=ITEMS[-1]):
    return random_dcn(*head, user_num, item_num, seed)


def second_realisation(w, users, head, eps=EPS):
    """The eval-mode DCN in fp32 numpy BY THE COLLAPSED FORM and in another order of sums -> [n, I]"""
    factor, L, C, ln = head
    f32 = np.float32
    w = {k: np.asarray(v, dtype=f32) for k, v in w.items()}
    n, n_items = len(users), len(w[ITEM_KEY])
    E = factor << L
    D = 2 * E
    # the deep net: layer 0 as the two products Pu and Pi added per pair, every later product over reversed columns
    p = "deep_net.layers.0."
    pu = w[USER_KEY][users] @ w[p + "linear.weight"][:, :E].T
    pi = w[ITEM_KEY] @ w[p + "linear.weight"][:, E:].T + w[p + "linear.bias"]
    a = (pu[:, None, :] + pi[None, :, :]).reshape(n * n_items, E)
    for l in range(L):
        p = f"deep_net.layers.{l}."
        if l:
            a = np.ascontiguousarray(h[:, ::-1]) @ np.ascontiguousarray(w[p + "linear.weight"][:, ::-1]).T + w[p + "linear.bias"]
        if ln:
            a = _ln(a, w[p + "layer_norm.weight"], w[p + "layer_norm.bias"], eps)[0]
        h = np.maximum(a, 0)
    wo = w[OUT_W].reshape(-1)
    z_deep = (np.ascontiguousarray(h[:, ::-1]) @ np.ascontiguousarray(wo[D:][::-1])).reshape(n, n_items)
    # the cross net: the scalars of the user rows and of the item rows, then the recurrence per pair
    _, K, B = dcn_score_constants(w, f32)
    su, si = dcn_row_scalars_host(w, w[USER_KEY][users], 0, f32), dcn_row_scalars_host(w, w[ITEM_KEY], 1, f32)
    d = su[:, None, 2:] + si[None, :, 2:]                    # [n, I, C + 1]
    if ln:
        mu_u, mu_i = su[:, None, 0], si[None, :, 0]
        m0 = (mu_u + mu_i) * f32(0.5)
        v0 = ((su[:, None, 1] + si[None, :, 1]) + f32(E) * ((mu_u - m0) ** 2 + (mu_i - m0) ** 2)) / f32(D)
        s = d[:, :, 0]
        for c in range(C):
            k = s + f32(1)
            t = k / np.sqrt(k * k * v0 + f32(eps))
            s = t * (d[:, :, c + 1] - m0 * K[c]) + B[c]
        z_cross = s
    else:
        m = np.ones((n, n_items), dtype=f32)
        for c in range(C):
            m = m * d[:, :, c] + f32(1)
        z_cross = m * d[:, :, C]
    z = (z_cross + z_deep) + w[OUT_B][0]
    assert z.dtype == f32
    return z


def case_ratios(x, o64, r32):
    """{(n, I): max|x - o64| / max(max|r32 - o64|, 2^-22 max|o64|)} over the blocks [:n, :I] of full-size rows"""
    out = {}
    for n in NS:
        for n_items in ITEMS:
            ref = o64[:n, :n_items]
            floor = max(np.abs(r32[:n, :n_items] - ref).max(), 2.0 ** -22 * np.abs(ref).max())
            out[(n, n_items)] = float(np.abs(x[:n, :n_items].astype(np.float64) - ref).max() / floor)
    return out


def yardsticks(w, users, eps=EPS):
    o64 = dcn_scores_host(w, users, None, np.float64, eps)
    r32 = dcn_scores_host(w, users, None, np.float32, eps)
    assert r32.dtype == np.float32
    return o64, r32.astype(np.float64)


def second_worst(head, seed, eps=EPS):
    """the largest ratio of second_realisation over the cases of the model of `seed`"""
    users = users_of()
    w = model_weights(head, seed)
    o64, r32 = yardsticks(w, users, eps)
    return max(case_ratios(second_realisation(w, users, head, eps), o64, r32).values())


@functools.lru_cache(maxsize=None)
def world(head, eps=EPS):
    """The model of SEEDS[head], the users and the two yardsticks at the largest size; computed once, shared, never written"""
    users = users_of()
    w = model_weights(head, SEEDS[head])
    o64, r32 = yardsticks(w, users, eps)
    for a in list(w.values()) + [users, o64, r32]:
        a.setflags(write=False)
    return dict(head=head, w=w, users=users, o64=o64, r32=r32)


def tensors(w, device="cuda"):
    """`w` as torch tensors on `device` (copies: the shared arrays are read-only)"""
    import torch
    return {k: torch.from_numpy(np.array(v)).to(device) for k, v in w.items()}


if __name__ == "__main__":                                   # the choice of SEEDS
    found = {}
    for head in HEADS:
        for seed in range(FIRST_SEED, FIRST_SEED + 200):
            worst = second_worst(head, seed)
            print(head, "seed", seed, f"the second realisation: largest ratio {worst:.2f}")
            if worst <= C_BOUND:
                found[head] = seed
                break
    print("SEEDS =", found)
