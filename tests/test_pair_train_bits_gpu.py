"""The outputs of the pair-head training entries (pmgt_ncf_train_grad / _table / _dropout / _rows, pmgt_ncf_model_train_grad,
pmgt_dcn_forward / _train_grad / _train_grad_dropout) pinned BIT FOR BIT: the operator tests hold the kernels to four times the fp32
formula's error, which a reordered sum passes or fails by luck.  tests/golden/pair_train_bits.json was recorded on an MI355X from the
commit BEFORE ops/ncf_train.hip, ops/ncf_model_train.hip and ops/dcn_train.hip came to share ops/pair_train_tile.h: that commit's three
files plus pair_train_bits_util.py (run as a script) and this file, nothing else.  A differing output hash means a floating-point
operation moved, and the answer is to fix the kernel, never to record again."""
import json
import os

import pytest

from tests.pair_train_bits_util import CASES, run_case

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pair_train_bits.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_fixture_holds_every_case():
    assert sorted(GOLDEN) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_the_outputs_keep_their_bits(name):
    inputs, outputs = run_case(name)
    assert inputs == GOLDEN[name]["input"], f"{name}: the generator changed (the inputs are not the recorded ones)"
    assert outputs == GOLDEN[name]["output"], f"{name}: the outputs differ from the recorded bits"
