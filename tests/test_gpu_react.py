"""GPU suite (-m gpu) for the reactive transport step: the cases of test_react_emulation.py on the gfx950 HIP library."""
import pytest

import porepy_amd as pa
from tests import _react_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


@pytest.mark.parametrize("n,k", [(3, 4), (4, 4), (3, 3), (4, 3), (3, 8), (4, 8)])
def test_exact_against_the_whole_system(lib, n, k):
    C.exact(lib, n, k)


def test_reduces_to_independent_components(lib):
    C.reduces_to_components(lib)


def test_chain_on_the_line_closed_form(lib):
    C.closed_form(lib)


def test_immobile_partner(lib):
    C.immobile_partner(lib)


def test_conservation(lib):
    C.conservation(lib)


def test_positivity(lib):
    C.positivity(lib)


def test_launch_forms_and_determinism(lib):
    C.launch_forms(lib)


@pytest.mark.parametrize("which", ["cyclic12", "rotation8", "cyclic12-k3"])
def test_cyclic_core(lib, which):
    C.core_case(lib, which)


def test_refusals(lib):
    C.refusals(lib)


def test_handle(lib):
    C.handle(lib)
