"""The scores of pmgt_ncf_score, pmgt_ncf_model_score and pmgt_dcn_score pinned BIT FOR BIT: the operator tests hold the kernels to four
times the fp32 formula's error, which a reordered sum passes.  tests/golden/score_tower_bits.json was recorded on an MI355X from the
commit BEFORE the three files came to share one tower (score_bits_util.py run as a script); a differing output hash means a
floating-point operation moved, and the answer is to fix the kernel, not to record again."""
import json
import os

import pytest

from tests.score_bits_util import CASES, run_case

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_tower_bits.json")) as _f:
    GOLDEN = json.load(_f)


def test_the_fixture_holds_every_case():
    assert sorted(GOLDEN) == sorted(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_the_scores_keep_their_bits(name):
    inputs, outputs = run_case(name)
    assert inputs == GOLDEN[name]["input"], f"{name}: the generator changed (the inputs are not the recorded ones)"
    assert outputs == GOLDEN[name]["output"], f"{name}: the scores differ from the recorded bits"
