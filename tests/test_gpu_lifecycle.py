"""GPU suite (-m gpu) for the life cycle of the active system: the cases of test_lifecycle_emulation.py on the gfx950
HIP library, plus the outputs of the calls with the vectors on the device."""
import pytest

import porepy_amd as pa
from tests import _lifecycle_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


def _to_device(a):
    import torch

    t = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    return t.data_ptr(), t


def _to_host(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("precond,windows", C.WALKS)
def test_walk_leaves_nothing_stale(lib, precond, windows):
    C.walk(lib, precond, windows)


@pytest.mark.parametrize("which", ["transport", "advdiff"])
def test_advance_step_that_does_not_converge(lib, which):
    print(C.advance_not_converged(lib, which))


def test_device_outputs_equal_the_host_ones(lib):
    C.device_outputs(lib, _to_device, _to_host)
