"""The result bits of the guided, person and row steps and of the three pack kernels against tests/golden/step_bits.json, SHA-256 digests
recorded once (tools/gpu_step_bits.py) from a library built from the sources of the commit before the kernels came to share their
bodies: the three entries are compared with that commit, not only with each other."""
import json
import os

import pytest

from tests.step_bits_support import CASES, digests, run

pytestmark = pytest.mark.gpu

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "step_bits.json")) as f:
    GOLDEN = json.load(f)


def test_the_recording_holds_the_case_list():
    assert sorted(GOLDEN["cases"]) == sorted(CASES) and len(set(CASES)) == len(CASES)


@pytest.mark.parametrize("name", CASES)
def test_the_bits_are_the_recorded_ones(name):
    """The updated latents and the whole `work` buffer (pre-filled: regions a launch must not touch are covered), or a pack kernel's output."""
    assert digests(run(name, "cuda")) == GOLDEN["cases"][name]
