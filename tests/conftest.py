"""pytest configuration: the ``gpu`` marker, the repo root on sys.path and MKL's code path pinned."""
import os
import sys

# The oracle tests compare torch-CPU results bit for bit with fixtures captured from the reference.  MKL (torch's exp,
# einsum / bmm) picks its code path by CPU, and the last bits differ between paths.  Pinned to the AVX2 branch in
# strict mode, the one tests/golden/make_golden.py captures the fixtures under, the path on Intel CPUs no longer
# depends on which instruction sets the CPU has.  MKL on AMD CPUs takes its own exp path whatever the pin, so the
# bit-exact fixture tests (G1, G6 and two G9 cases) do not hold there.  It has to be set before MKL's first call.
os.environ["MKL_CBWR"] = "AVX2,STRICT"

import numpy as np  # noqa: E402
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def golden(name):
    """Load one fixture captured from the reference by tests/golden/make_golden.py."""
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="session")
def load_golden():
    return golden
