"""GPU suite (-m gpu) for the adjoint of the saturation step: the cases of test_saturation_adjoint_emulation.py on the
gfx950 HIP library."""
import pytest

import porepy_amd as pa
from tests import _saturation_adjoint_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


@pytest.mark.parametrize("n", [3, 4])
def test_exact_against_the_judge(lib, n):
    C.exact(lib, n)


def test_table_and_linear(lib):
    C.table_and_linear(lib)


def test_flat_cells(lib):
    C.flat_cells(lib)


def test_line_closed_form(lib):
    C.line_closed_form(lib)


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
