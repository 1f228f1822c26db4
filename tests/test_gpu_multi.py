"""GPU suite (-m gpu) for the multi-component transport step: the cases of test_multi_emulation.py on the gfx950 HIP
library."""
import pytest

import porepy_amd as pa
from tests import _multi_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


@pytest.mark.parametrize("n,k", [(4, 1), (4, 3), (4, 8), (3, 3)])
def test_exact_against_spsolve(lib, n, k):
    C.exact(lib, n, k)


def test_implicit_euler_closed_form(lib):
    C.closed_form(lib)


def test_agrees_with_single_runs(lib):
    C.agrees_with_single_runs(lib, 4, 3)


def test_deterministic_and_merged_form(lib):
    C.deterministic_and_merged(lib, 6, 3)


def test_a_core_takes_the_component_path(lib):
    C.core_takes_the_component_path(lib)


def test_jacobi_takes_the_component_path(lib):
    C.jacobi_takes_the_component_path(lib)


def test_failed_check_falls_back(lib):
    C.failed_check_falls_back(lib)


def test_errors(lib):
    C.errors(lib)


def test_lifetime(lib):
    C.lifetime(lib)


def test_flow_system_is_untouched(lib):
    C.flow_system_is_untouched(lib)
