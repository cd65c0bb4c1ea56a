"""GPU: the bits of the PCG iterates x_k that libpgo.so returns on the cases of tests/pcg_bits_cases.py against tests/golden/pcg_kernel_bits.json, which
scripts/record_pcg_kernel_bits.py wrote from the library as it stood before the PCG kernels' shared statements moved into csrc/pgo_pcg_ops.hpp.  No tolerance: no
form of the iteration has atomics and every sum has a fixed order, so a change that is not meant to alter a number leaves every digest as it is."""
import json
import os

import pytest

from tests import pcg_bits_cases as cases

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pcg_kernel_bits.json")


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def test_the_recording_holds_these_cases(recorded):
    assert sorted(recorded) == sorted(cases.CASE_NAMES)


@pytest.mark.parametrize("name", cases.CASE_NAMES)
def test_the_library_returns_the_recorded_bits(recorded, name):
    got, want = cases.digests(name), recorded[name]
    assert got["inputs"] == want["inputs"], "inputs differ from the recording"
    differ = [k for k in want["outputs"] if got["outputs"].get(k) != want["outputs"][k]]
    print("PCG bits %-44s %d outputs, differing: %s" % (name, len(want["outputs"]), differ or "none"))
    assert sorted(got["outputs"]) == sorted(want["outputs"]) and not differ
