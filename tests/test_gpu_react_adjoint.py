"""GPU suite (-m gpu) for the adjoint of the reactive transport step: the cases of test_react_adjoint_emulation.py on
the gfx950 HIP library."""
import pytest

import porepy_amd as pa
from tests import _react_adjoint_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


def test_judge_formulas_against_complex_step(lib):
    C.formulas_against_complex_step(lib)


@pytest.mark.parametrize("n,k", [(3, 3), (3, 4), (3, 8), (4, 1), (4, 3), (4, 4), (4, 8)])
def test_exact_against_the_judge(lib, n, k):
    C.exact(lib, n, k)


def test_reduces_to_the_uncoupled_adjoint(lib):
    C.reduces_to_uncoupled(lib)


def test_immobile_partner(lib):
    C.immobile_partner(lib)


def test_adjoint_identity_with_own_forward(lib):
    C.identity_with_own_forward(lib)


def test_line_closed_form(lib):
    C.line_closed_form(lib)


def test_launch_forms_and_determinism(lib):
    C.launch_forms_and_determinism(lib)


@pytest.mark.parametrize("name", ["cyclic12", "rotation8"])
def test_cyclic_core(lib, name):
    C.cyclic_core(lib, name)


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
