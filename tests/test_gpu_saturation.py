"""GPU suite (-m gpu) for the saturation step: the cases of test_saturation_emulation.py on the gfx950 HIP library."""
import pytest

import porepy_amd as pa
from tests import _saturation_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


@pytest.mark.parametrize("n,kind", [(3, "corey"), (3, "table"), (4, "corey"), (4, "table")])
def test_exact_against_global_newton(lib, n, kind):
    C.exact(lib, n, kind)


@pytest.mark.parametrize("n_w,n_n,wells", [(2.0, 2.0, False), (3.0, 1.5, False), (2.0, 2.0, True), (3.0, 1.5, True)])
def test_line_against_its_recursion(lib, n_w, n_n, wells):
    C.line_case(lib, n_w, n_n, wells)


def test_linear_kind_is_the_linear_step(lib):
    C.linear_kind_is_the_linear_step(lib)


@pytest.mark.parametrize("which", ["cyclic12", "rotation8"])
def test_core_converges(lib, which):
    C.core_converges(lib, which)


def test_deterministic_and_merged_form(lib):
    C.deterministic_and_merged(lib)


def test_leaves_the_interval(lib):
    C.leaves_the_interval(lib)


def test_errors(lib):
    C.errors(lib)


def test_lifetime(lib):
    C.lifetime(lib)


def test_flow_system_is_untouched(lib):
    C.flow_system_is_untouched(lib)
