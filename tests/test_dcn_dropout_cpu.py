"""The DCN in training mode on the host: dcn_head_grad_host(masks=) against fp64 autograd through pmgt_amd.dcn.DCN ITSELF, its Dropout
modules replaced by stubs that multiply by the given masks (so the place of every dropout -- before the LayerNorm in the deep net, on
x0 s_c alone in the cross net -- is the model's, not a restatement's); masks=None keeps the bits of the call without the argument; the
masks are those of the project's one RNG and keep the stated fraction; and the measure of tests/test_dcn_dropout_grad_gpu.py, checked with
a SECOND fp32 realisation (torch autograd under the stub masks) before any device takes it: FLOOR_FACTOR stays 1."""
import re

import numpy as np
import pytest
import torch

from pmgt_amd import _lib
from pmgt_amd.dcn_head import dcn_dropout_masks, dcn_head_grad_host
from pmgt_amd.ncf_head import ncf_dropout_keep
from tests.dcn_dropout_util import (NS, PS, SEED, abs_grad_masked, cut, degenerate_keys_p, host_masked, masks_of, near_keys_p,
                                    second_realisation, torch_grad_masked, world)
from tests.dcn_util import C_BOUND, EPS, HEADS, degenerate_keys, head_id

CASES = [(8, 2, 3, True), (8, 2, 3, False), (16, 1, 4, True)]


@pytest.mark.parametrize("shape", CASES, ids=head_id)
def test_the_masked_host_gradient_is_fp64_autograd_through_the_model_with_stub_masks(shape):
    h = world(shape if shape in HEADS else (8, 2, 3, True))
    if shape not in HEADS:                                   # (8, 2, 3, off): the LayerNorm tensors of the seeded model left out
        h = dict(h, w={k: v for k, v in h["w"].items() if "layer_norm" not in k})
    n = 33
    users, items, labels = h["users"][:n], h["items"][:n], h["labels"][:n]
    for p in PS + [(0.3, [0.5, 0.0, 0.2, 0.4][:shape[1]], [0.0, 0.6, 0.1, 0.3, 0.0, 0.2][:shape[2]])]:      # the last: p's differ per layer
        masks = masks_of(shape, n, p, 7)
        got = host_masked(h["w"], users, items, labels, np.float64, masks)
        want = torch_grad_masked(h["w"], shape, users, items, labels, masks, torch.float64)
        assert sorted(got) == sorted(want)
        for k in got:
            assert np.abs(got[k] - want[k].reshape(got[k].shape)).max() <= 1e-12, (p, k)
        assert not np.array_equal(got["logits"], host_masked(h["w"], users, items, labels, np.float64, None)["logits"])


@pytest.mark.parametrize("shape", CASES[::2], ids=head_id)
def test_no_masks_keeps_the_bits(shape):
    h = world(shape)
    users, items, labels = h["users"][:33], h["items"][:33], h["labels"][:33]
    for dtype in (np.float64, np.float32):
        a = dcn_head_grad_host(h["w"], users, items, labels, dtype, layer_norm_eps=EPS)
        b = dcn_head_grad_host(h["w"], users, items, labels, dtype, layer_norm_eps=EPS, masks=None)
        keep_all = host_masked(h["w"], users, items, labels, dtype, masks_of(shape, 33, (0.0, 0.0, 0.0), 3))
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
        assert all(a[2][k].tobytes() == b[2][k].tobytes() for k in a[2]) and sorted(a[2]) == sorted(b[2])
        assert all(np.array_equal(a[2][k], keep_all[k]) for k in a[2])      # p = 0: every mask is all ones with the scale 1


def test_the_masks_are_the_project_s_rng_at_sites_of_their_own_and_keep_the_stated_fraction():
    assert len({_lib.DCN_SITE_EMB} | {_lib.DCN_SITE_DEEP + l for l in range(_lib.DCN_MAX_DEEP)}
               | {_lib.DCN_SITE_CROSS + c for c in range(_lib.DCN_MAX_CROSS)}) == 1 + _lib.DCN_MAX_DEEP + _lib.DCN_MAX_CROSS
    hdr = open(__file__.replace("tests/test_dcn_dropout_cpu.py", "include/pmgt_capi.h")).read()
    src = open(__file__.replace("tests/test_dcn_dropout_cpu.py", "pmgt_amd/ops/ncf_head.h")).read()
    assert "pmgt_dcn_train_grad_dropout(" in hdr and "pmgt_dcn_train_grad_dropout" in _lib.HIP_SYMBOLS
    assert f"DCN_SITE_EMB = {_lib.DCN_SITE_EMB}, DCN_SITE_DEEP = {_lib.DCN_SITE_DEEP}, DCN_SITE_CROSS = {_lib.DCN_SITE_CROSS};" in src
    for name, value in (("DCN_SITE_EMB", _lib.DCN_SITE_EMB), ("DCN_SITE_DEEP", _lib.DCN_SITE_DEEP), ("DCN_SITE_CROSS", _lib.DCN_SITE_CROSS)):
        assert re.search(rf"{name} +{value}\b", hdr), name
    n, rows, cols = 130, 130, 512
    for p in (0.2, 0.5, 0.8):
        m = dcn_dropout_masks(SEED, 7, n, 64, 2, 3, p, p, p)
        assert sorted(m) == ["cross0", "cross1", "cross2", "deep0", "deep1", "emb"]
        assert m["emb"][0].shape == (n, 512) and m["deep0"][0].shape == (n, 256) and m["deep1"][0].shape == (n, 128) and m["cross2"][0].shape == (n, 512)
        assert np.array_equal(m["emb"][0], ncf_dropout_keep(SEED, 7, _lib.DCN_SITE_EMB, n, 512, p))
        assert np.array_equal(m["deep1"][0], ncf_dropout_keep(SEED, 7, _lib.DCN_SITE_DEEP + 1, n, 128, p))
        assert np.array_equal(m["cross2"][0], ncf_dropout_keep(SEED, 7, _lib.DCN_SITE_CROSS + 2, n, 512, p))
        assert m["emb"][1] == np.float32(1) / (np.float32(1) - np.float32(p)) and m["emb"][1].dtype == np.float32
        sigma = np.sqrt(p * (1 - p) / (rows * cols))
        for k in ("emb", "cross0", "cross1", "cross2"):      # 130 x 512: within 4 binomial sigmas of 1 - p
            assert abs(m[k][0].mean() - (1 - p)) <= 4 * sigma, (p, k, m[k][0].mean())
        assert not np.array_equal(m["cross0"][0], m["cross1"][0]) and not np.array_equal(m["emb"][0], m["cross0"][0])
        assert not np.array_equal(m["emb"][0], dcn_dropout_masks(SEED, 8, n, 64, 2, 3, p, p, p)["emb"][0])
    assert np.array_equal(cut(m, 31)["emb"][0], dcn_dropout_masks(SEED, 7, 31, 64, 2, 3, 0.8, 0.8, 0.8)["emb"][0])      # a row is the pair's index
    with pytest.raises(ValueError, match="outside"):
        dcn_dropout_masks(SEED, 0, 4, 8, 2, 3, 1.0, 0.0, 0.0)
    with pytest.raises(ValueError, match="cross dropouts"):
        dcn_dropout_masks(SEED, 0, 4, 8, 2, 3, 0.1, 0.0, [0.1, 0.2])


def test_the_degenerate_set_depends_on_the_cross_dropouts():
    shape = (8, 2, 3, True)
    assert degenerate_keys_p(shape, 0.0) == degenerate_keys(shape) and degenerate_keys_p((8, 2, 3, False), 0.0) == []
    assert degenerate_keys_p(shape, 0.5) == []
    # layer 2 draws nothing: nothing below it has a gradient; layers 1 and 2 draw: only layer 0's w is left
    assert sorted(degenerate_keys_p(shape, [0.0, 0.5, 0.0])) == sorted(degenerate_keys(shape))
    assert degenerate_keys_p(shape, [0.0, 0.5, 0.5]) == ["cross_net.layers.0.weight"]
    assert sorted(near_keys_p(shape, 0.5)) == sorted(degenerate_keys(shape)) and near_keys_p(shape, 0.0) == []
    h = world(shape)
    users, items, labels = h["users"][:33], h["items"][:33], h["labels"][:33]
    for p_cross in (0.0, [0.0, 0.5, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5], 0.5):
        masks = masks_of(shape, 33, (0.2, 0.3, p_cross), 0)
        o64, mags = host_masked(h["w"], users, items, labels, np.float64, masks), abs_grad_masked(h["w"], users, items, labels, masks)
        for k in o64:
            if k == "logits":
                continue
            assert (np.abs(o64[k]) <= mags[k].reshape(o64[k].shape) * (1 + 1e-9) + 1e-300).all(), k      # the magnitudes bound the values
            small = np.abs(o64[k]).max() < 2.0 ** -22 * np.abs(mags[k]).max()
            assert small == (k in degenerate_keys_p(shape, p_cross)), (p_cross, k)


@pytest.mark.parametrize("shape", HEADS, ids=head_id)
def test_a_second_fp32_realisation_passes_the_measure_under_the_masks(shape):
    """torch autograd in fp32 under the stub masks against the measure of the GPU test, every case of it, with A FACTOR 2 TO SPARE on the
    nearly degenerate and on the degenerate tensors: NEAR_FLOOR_FACTOR 16 and FLOOR_FACTOR 1 hold (tests/dcn_dropout_util.py)."""
    h = world(shape)
    for n in NS:
        assert h["redrawn"][:n].sum() * 8 <= n               # at most 1 pair in 8 was drawn again
    near, rest, dead = second_realisation(shape, h)
    print(f"{head_id(shape)}: largest ratio {rest:.2f}, of a nearly degenerate tensor {near:.2f}, degenerate error / floor {dead:.2f}")
    assert rest <= C_BOUND and near <= C_BOUND / 2 and dead <= 2.0
