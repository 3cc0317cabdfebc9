"""The measure of the NCF-model GPU tests, checked on the CPU before any kernel is judged by it: a SECOND fp32 realisation of the yardstick
(torch autograd through pmgt_amd.ncf.NCF) must pass  max|x - o64| <= 4 max(max|r32 - o64|, 2^-22 max|o64|)  on every case of
tests/test_ncf_model_grad_gpu.py (a pair list on which a right realisation misses the bound cannot judge a kernel), and every pair list of
that file -- eval mode, under the dropout mask sets, the 65 536 pairs -- keeps within the cap of 1 pair in 8 drawn again."""
import numpy as np
import pytest

from tests.dcn_util import C_BOUND, ratios
from tests.ncf_model_util import (DROP_HEADS, HEADS, NS, OTHER_HEADS, cut, drop_world, head_id, host, label_sets, masks_of, other_orders,
                                  permuted_host, second_realisation_masked, torch_grad, world)


@pytest.mark.parametrize("h", HEADS, ids=head_id)
def test_a_second_fp32_realisation_passes_the_measure_on_every_case(h):
    hw = world(h)
    worst = 0.0
    for n in NS:
        for name, labels in label_sets(hw, n):
            users, items = hw["users"][:n], hw["items"][:n]
            o64, r32 = (host(hw["w"], hw["kind"], users, items, labels, dt) for dt in (np.float64, np.float32))
            rt = ratios(torch_grad(hw["w"], h, users, items, labels), o64, r32)
            assert sorted(rt) == sorted(o64)
            bad = {k: v for k, v in rt.items() if not v <= C_BOUND}
            assert not bad, (h, n, name, bad)
            worst = max(worst, max(rt.values()))
    print(f"{head_id(h)}: torch fp32 against the measure, largest ratio {worst:.2f}")
    worst, where = other_orders(h, hw, False)
    print(f"{head_id(h)}: the yardstick in other orders of sums, largest ratio {worst:.2f} at {where}")
    assert worst <= C_BOUND


@pytest.mark.parametrize("h", DROP_HEADS, ids=head_id)
def test_a_second_fp32_realisation_passes_the_measure_under_every_mask_set(h):
    hw = drop_world(h)                                       # (world asserts the cap and the two conditions of its header for every n of NS)
    assert all(hw["redrawn"][:n].sum() * 8 <= n for n in NS)
    worst = second_realisation_masked(h, hw)
    print(f"{head_id(h)}: torch fp32 under the masks against the measure, largest ratio {worst:.2f}")
    assert worst <= C_BOUND
    worst, where = other_orders(h, hw, True)
    print(f"{head_id(h)}: the yardstick in other orders of sums under the masks, largest ratio {worst:.2f} at {where}")
    assert worst <= C_BOUND


def test_the_permuted_yardstick_is_the_yardstick_in_fp64():
    for h in (HEADS[1], HEADS[5]):
        hw, n = drop_world(h), 33
        masks = cut(masks_of(h, NS[-1], 0.3, [0.1, 0.5], 7), n)
        args = (hw["users"][:n], hw["items"][:n], hw["labels"][:n])
        a, b = host(hw["w"], hw["kind"], *args, np.float64, True, masks), permuted_host(hw["w"], h, *args, masks, np.float64)
        assert sorted(a) == sorted(b) and all(np.abs(a[k] - b[k]).max() <= 1e-12 for k in a)


def test_every_pair_list_of_the_gpu_tests_keeps_the_cap():
    for shape in OTHER_HEADS:
        world(shape)
    hw = world((8, 2, "NeuMF-end", True), 3000, 5000, 65536, seed=23)
    assert hw["redrawn"].sum() * 8 <= 65536
