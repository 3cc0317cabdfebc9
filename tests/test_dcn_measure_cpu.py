"""The measure of tests/test_dcn_grad_gpu.py, checked on the CPU before any device takes it: a SECOND fp32 realisation of the yardstick --
torch autograd through pmgt_amd.dcn.DCN, whose LayerNorm, matrix products and sums run in other orders than numpy's -- must pass the same
assertion with the same constant on every case of the operator test,
    max|t32 - o64| <= 4 max(max|r32 - o64|, floor),   floor = 2^-22 max|o64|, for the degenerate tensors FLOOR_FACTOR 2^-22 M
(tests/dcn_util.py).  FLOOR_FACTOR is the smallest power of two at which both pass
WITH A FACTOR 2 TO SPARE on the degenerate tensors (error <= 2 floor): it is 1.  Measured here: the largest error of a degenerate tensor, of either
realisation, is 0.06 floor; the largest ratio of any quantity per head is 1.53, 1.89, 1.47, 2.72, 2.05, 1.70.
Also checked: the pair lists of the operator test draw at most 1 pair in 8 again (none, at the seeds chosen)."""
import numpy as np
import pytest

from tests.dcn_util import C_BOUND, FLOOR_FACTOR, HEADS, NS, abs_grad, degenerate_keys, head_id, host, label_sets, ratios, torch_grad, world


@pytest.mark.parametrize("shape", HEADS, ids=head_id)
def test_a_second_fp32_realisation_passes_the_measure(shape):
    h = world(shape)
    worst_t, worst_floor = {}, 0.0
    for n in NS:
        for name, labels in label_sets(h, n):
            users, items = h["users"][:n], h["items"][:n]
            o64, r32 = host(h["w"], users, items, labels, np.float64), host(h["w"], users, items, labels, np.float32)
            t32 = torch_grad(h["w"], shape, users, items, labels)
            mags = abs_grad(h["w"], users, items, labels)
            assert sorted(t32) == sorted(o64) == sorted(list(mags) + ["logits"])
            for k, v in ratios(t32, o64, r32, shape, mags).items():
                worst_t[k] = max(worst_t.get(k, 0.0), v)
            for k in degenerate_keys(shape):
                floor = FLOOR_FACTOR * 2.0 ** -22 * np.abs(mags[k]).max()
                assert np.abs(o64[k]).max() < 2.0 ** -22 * np.abs(mags[k]).max(), (k, "not degenerate")
                worst_floor = max(worst_floor, np.abs(t32[k].reshape(o64[k].shape) - o64[k]).max() / floor, np.abs(r32[k] - o64[k]).max() / floor)
    print(f"{head_id(shape)}: largest ratio {max(worst_t.values()):.2f}, degenerate error / floor {worst_floor:.2f}")
    assert max(worst_t.values()) <= C_BOUND, worst_t
    assert worst_floor <= 2.0                                # the factor 2 to spare


@pytest.mark.parametrize("shape", HEADS, ids=head_id)
def test_the_pair_lists_are_well_conditioned_with_few_redraws(shape):
    h = world(shape)
    for n in NS:
        assert h["redrawn"][:n].sum() * 8 <= n
    assert h["users"].max() == 3 and h["items"].max() == 5 and len(set(zip(h["users"].tolist(), h["items"].tolist()))) < len(h["users"])


def test_the_absolute_value_backward_bounds_the_gradient():
    h = world((8, 2, 3, True))
    users, items, labels = h["users"][:33], h["items"][:33], h["labels"][:33]
    o64, mags = host(h["w"], users, items, labels, np.float64), abs_grad(h["w"], users, items, labels)
    for k in o64:
        if k != "logits":
            assert (np.abs(o64[k]) <= mags[k].reshape(o64[k].shape) * (1 + 1e-9) + 1e-300).all(), k
