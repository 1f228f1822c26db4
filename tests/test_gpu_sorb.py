"""GPU suite (-m gpu) for the sorbing transport step: the cases of test_sorb_emulation.py on the gfx950 HIP library."""
import pytest

import porepy_amd as pa
from tests import _sorb_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


@pytest.mark.parametrize("name", list(C.ISOTHERMS))
@pytest.mark.parametrize("n", [3, 4])
def test_exact_on_an_acyclic_flux(lib, n, name):
    C.exact(lib, n, name)


@pytest.mark.parametrize("name", C.NONLINEAR)
def test_line_against_its_recursion(lib, name):
    C.line_case(lib, name)


def test_linear_is_the_linear_step_bit_for_bit(lib):
    C.linear_is_the_linear_step(lib)


@pytest.mark.parametrize("k,solo", [(5, (0, 1, 2, 3, 4)), (64, (63, 0))])
def test_components_do_not_see_each_other(lib, k, solo):
    C.independent(lib, k, solo)


@pytest.mark.parametrize("which", ["cyclic12", "rotation8"])
def test_cyclic_core_converges(lib, which):
    C.core_converges(lib, which)


def test_deterministic_and_merged(lib):
    C.deterministic_and_merged(lib)


def test_mass(lib):
    C.mass(lib)


def test_no_non_negative_root(lib):
    C.no_root(lib)


def test_errors(lib):
    C.errors(lib)


def test_lifetime(lib):
    C.lifetime(lib)


def test_flow_system_is_untouched(lib):
    C.flow_system_is_untouched(lib)
