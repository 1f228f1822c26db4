"""CPU suite for the life cycle of the active system (one handle through every activating call, the advance calls'
failed step) on the host-emulation build; tests/test_gpu_lifecycle.py runs the same cases on the HIP library."""
import pytest

from tests import _lifecycle_cases as C
from tests import _parity as P


@pytest.fixture(scope="module")
def lib():
    return P.emulation_library()


@pytest.mark.parametrize("precond,windows", C.WALKS)
def test_walk_leaves_nothing_stale(lib, precond, windows):
    C.walk(lib, precond, windows)


@pytest.mark.parametrize("which", ["transport", "advdiff"])
def test_advance_step_that_does_not_converge(lib, which):
    print(C.advance_not_converged(lib, which))
