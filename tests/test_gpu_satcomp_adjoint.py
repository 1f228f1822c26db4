"""GPU suite (-m gpu) for the adjoint of the saturation step with phase-carried components: the cases of
test_satcomp_adjoint_emulation.py on the gfx950 HIP library."""
import pytest

import porepy_amd as pa
from tests import _satcomp_adjoint_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("n", [3, 4])
def test_exact_against_the_judge(lib, n, k):
    C.exact(lib, n, k)


def test_no_component_loads(lib):
    C.no_component_loads(lib)


def test_linear_constant_saturation(lib):
    C.linear_constant_saturation(lib)


def test_table(lib):
    C.table(lib)


@pytest.mark.parametrize("k", [2, 64])
def test_line(lib, k):
    C.line(lib, k)


@pytest.mark.parametrize("name", ["cyclic12", "rotation8"])
def test_cyclic_core(lib, name):
    C.cyclic_core(lib, name)


def test_own_forward_differences(lib):
    C.own_forward_differences(lib)


def test_launch_forms_and_determinism(lib):
    C.launch_forms_and_determinism(lib)


def test_observation_forms(lib):
    C.observation_forms(lib)


def test_refusals(lib):
    C.refusals(lib)


def test_handle(lib):
    C.handle(lib)


def test_flow_system_is_untouched(lib):
    C.flow_system_is_untouched(lib)


def _to_device(a):
    import torch

    t = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    return t.data_ptr(), t


def test_device_vectors(lib):
    C.device_vectors(lib, _to_device, lambda t: t.cpu().numpy())
