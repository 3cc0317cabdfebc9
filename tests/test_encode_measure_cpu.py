"""The yardstick of the inference measure (tests/encode_measure_util.py), settled on the CPU without the code under test.

(a) SECOND REALISATION.  For every case of tests/test_encode_measure_gpu.py the oracle under torch.autocast("cpu", bfloat16) with fp32
    parameters and the modality attention in fp32 (bf16_measure_util._Fp32ModalityAttention) -- another bf16 implementation whose rounding
    points are not the hook's -- must pass `forward_ratios` against (o64, e16): the chosen inputs keep an independent reference inside
    the bound before any GPU run.  Largest ratio per case (one run): headline table mode Tseq 1 / 2 / 3 0.79, 255 .. 258 0.87; token mode
    0.72 / 0.68 / 0.71, 255 .. 258 0.81; beta = 1 0.82; no mask 0.80 / 0.82; feats 0.71 / 0.81; probabilities at S 32 1.32, at d 128 /
    S 65 1.51; d = 512 1.09 at both counts; I = 4 d 0.93.  All a CLS row or hidden_states.0; with probabilities, probs.0 max-abs.
    The engine's own figures are in the GPU file's header.
(b) SLICING.  The references are computed at a world's largest sequence count and sliced; the reference of the sliced inputs agrees to
    fp64 rounding (1e-12 of the largest element), and the masked-key probabilities of every reference are exactly 0.
(c) NEGATIVE CONTROLS.  The truth mis-stated at beta = 0.53 against a realisation at 0.5: the measure rejects it on the probabilities
    (ratios 11.9 / 9.5 on probs.0 max / l2).  It does NOT on the hidden states -- with po.synth_params both softmaxes are close to uniform
    and three points of beta move the states by less than bf16 noise (largest hidden-state ratio 1.44 at 258 sequences) -- which is why
    the control lives in the case that measures probabilities (the hidden-state figure is printed, not asserted).  One sequence's rows overwritten with its
    neighbour's: the CLS-row kind rejects it (ratio 207 / 165 for sequence 0 / 1 of 257), and so do the global max and L2 kinds alone
    (cls max 89, l2 above 4 as well): a whole wrong sequence is an O(1) error against noise of 4e-3, not something only a per-row
    kind can see."""
import numpy as np
import pytest
import torch

from tests import encode_measure_util as em


@pytest.fixture(scope="module", autouse=True)
def release_the_references_with_the_module():
    yield
    for cached in (em.reference, em.world, em.misstated_truth):
        cached.cache_clear()


def realisation(label):
    c = em.CASES[label]
    return em.take(em.reference(c["world"], "ac"), c["T"])


@pytest.mark.parametrize("label", list(em.CASES))
def test_an_independent_bf16_realisation_passes_the_forward_measure(label):
    w, n_seq, o64, e16, mask = em.case_truth(label)
    rt = em.forward_ratios(realisation(label), o64, e16, mask)
    print(f"encode measure, autocast oracle {label}: {n_seq} sequences, {len(rt)} ratios, worst {em.worst(rt)}")
    L = w["cfg"]["num_hidden_layers"]
    want = 2 * (L + 3) + 1 + (3 if mask is not None else 2) * (L if w["probs"] else 0)
    assert len(rt) == want, sorted(rt)
    assert not em.failing(rt), em.failing(rt)
    # the yardstick is bf16 noise, not more: e16 within 2 % of the norm of every hidden state
    for k, v in o64.items():
        if not k.startswith("probs."):
            assert np.linalg.norm(e16[k] - v) < 2e-2 * np.linalg.norm(v), k


@pytest.mark.parametrize("name", ["tab", "probs", "d128_s65"])
def test_a_sliced_reference_is_the_reference_of_the_sliced_inputs(name):
    w = em.world(name)
    n_seq = 2
    part = em.run_oracle(w, ids=w["ids"][:n_seq], mask=w["mask"][:n_seq])
    for k, v in em.take(em.reference(name, "o64"), n_seq).items():
        assert np.abs(part[k] - v).max() <= 1e-12 * np.abs(v).max(), k


@pytest.mark.parametrize("name", ["probs", "d128_s65"])
def test_masked_keys_have_probability_zero_in_every_reference_and_the_measure_sees_one_that_has_not(name):
    w = em.world(name)
    o64 = em.reference(name, "o64")
    assert float((w["mask"] == 0).float().mean()) > 0.2 and bool((w["mask"][:, 0] == 1).all())
    for kind in ("o64", "e16", "e16_node", "r32", "ac"):
        rt = em.forward_ratios(em.reference(name, kind), o64, em.reference(name, "e16"), w["mask"])
        assert [v for k, v in rt.items() if k.endswith(":masked")] == [0.0] * w["cfg"]["num_hidden_layers"], kind
    bad = {k: np.array(v, copy=True) for k, v in em.reference(name, "e16").items()}
    bad["probs.0"][1, 0, 0, w["S"] - 1] = 1e-30                        # sequence 1 keeps position 0 alone
    rt = em.forward_ratios(bad, o64, em.reference(name, "e16"), w["mask"])
    assert em.failing(rt) == {"probs.0:masked": float("inf")}


def test_the_hook_hands_back_the_probabilities_from_before_their_rounding():
    """e16's probabilities are what the engine reports (fp32 registers before the pack to bf16): not bf16 values, and rows that sum to 1
    to fp64 rounding, which rounded probabilities do not"""
    e16 = em.reference("probs", "e16")
    p = e16["probs.0"]
    assert not np.array_equal(p, torch.from_numpy(p).to(torch.bfloat16).double().numpy())
    assert np.abs(p.sum(-1) - 1).max() < 1e-12


def test_negative_control_a_truth_misstated_at_beta_053_fails_the_measure_on_the_probabilities():
    o64, e16 = em.misstated_truth("probs")
    w = em.world("probs")
    rt = em.forward_ratios(em.reference("probs", "ac"), o64, e16, w["mask"])
    print(f"encode measure, negative control beta 0.53: worst {em.worst(rt, 5)}")
    bad = em.failing(rt)
    for l in range(w["cfg"]["num_hidden_layers"]):
        assert f"probs.{l}:max" in bad and f"probs.{l}:l2" in bad, bad
    o64, e16 = em.misstated_truth("tok")                              # reported, not asserted: what the hidden states alone make of it
    print(f"    hidden states only, 258 sequences: worst {em.worst(em.forward_ratios(em.reference('tok', 'ac'), o64, e16), 2)}")


@pytest.mark.parametrize("n_seq", [3, 257])
@pytest.mark.parametrize("r", [0, 1])
def test_negative_control_a_sequence_with_its_neighbours_rows_fails_the_cls_row_kind(n_seq, r):
    o64, e16 = em.yardstick("tok", n_seq, "bf16")
    rt = em.forward_ratios(em.with_neighbours_rows(em.take(em.reference("tok", "ac"), n_seq), r), o64, e16)
    print(f"encode measure, negative control sequence {r} of {n_seq} mis-paired: worst {em.worst(rt, 4)}; cls max {rt['cls:max']:.1f} "
          f"l2 {rt['cls:l2']:.1f} row {rt['cls:row']:.1f}")
    assert rt["cls:row"] > 10 * em.C_BOUND
    assert em.kinds_failing(rt) == ["l2", "max", "row"]              # reported as found: the global kinds see a whole wrong sequence too
