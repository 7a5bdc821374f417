import os
import sys

# Before anything calls MKL: its vector math (torch-CPU exp / tanh / ...) rounds differently per CPU vendor and ISA, and
# the bit-exact host tests compare against fixtures written in its COMPATIBLE branch, the same on every x86 host
# (tests/golden/gen_golden.py)
os.environ["MKL_CBWR"] = "COMPATIBLE"

import numpy as np  # noqa: E402
import pytest  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


@pytest.fixture(scope="session")
def golden():
    cache = {}

    def load(name):
        if name not in cache:
            cache[name] = np.load(os.path.join(GOLDEN, name + ".npz"))
        return cache[name]

    return load


@pytest.fixture(scope="session")
def oracle_mod():
    import oracle
    oracle.build()
    return oracle


def pytest_sessionfinish(session, exitstatus):
    """GPU sessions leave the measured parity errors behind (tests/_margins.py)."""
    import _margins
    if _margins.RECORDS or _margins.NOTES:
        out = os.path.join(ROOT, "gpurun_out")
        os.makedirs(out, exist_ok=True)
        _margins.dump(os.path.join(out, "parity_margins.txt"))
