"""Every image-stage call reproduces, bit for bit, what it computed before the stages were split into one translation unit each:
tests/image_pins.py runs the cases, tests/golden/image_stage_digests.json holds the SHA-256 of every output buffer and the exact
figures, recorded on an MI355X with the library of the commit before the split.  The suites of the single calls compare against
float64 references with a tolerance and would pass a last-bit change; this one does not."""
import pytest

import image_pins

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def got():
    return image_pins.digests()


@pytest.fixture(scope="module")
def want():
    return image_pins.golden()


def test_the_cases_are_the_recorded_ones(got, want):
    assert sorted(got) == sorted(want)
    assert {k.split("/")[0] for k in want} == set(image_pins.CALLS)


@pytest.mark.parametrize("call", image_pins.CALLS)
def test_reproduces_the_recorded_bits(got, want, call):
    cases = [k for k in want if k.split("/")[0] == call]
    assert cases
    bad = {k: (got.get(k), want[k]) for k in cases if got.get(k) != want[k]}
    assert not bad, f"{len(bad)} of {len(cases)} cases of {call} differ: {sorted(bad)[:8]}"
