"""The device sampler draws the ids (and reports the ``stats``) recorded in
tests/golden/sampling_draws.json, bit for bit: every summation order of the kernel is fixed
in its source, so a change of that source that moves one id changed what is computed.  The
cases, and why each reaches the path it is there for, are in tests/test_sampling_golden.py."""

import pytest

from test_sampling_golden import CASE_IDS, draw, golden

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", CASE_IDS)
def test_draws_match_golden(kernels, name):
    want = golden()["cases"][name]
    got = draw(name)
    assert got["ids"] == want["ids"]
    assert got.get("stats") == want.get("stats")
