"""GPU suite (-m gpu) for the flow-ordered sweep: the cases of test_sweep_emulation.py on the gfx950 HIP library."""
import pytest

import porepy_amd as pa
from tests import _sweep_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


@pytest.mark.parametrize("name", C.ORDER_CASES)
def test_order_parity(lib, name):
    C.order_parity(lib, name)


def test_stagnant_faces_make_no_edge(lib):
    C.stagnant_faces_make_no_edge(lib)


def test_direct_step_is_exact(lib):
    C.direct_step_exact(lib, 4)


def test_implicit_euler_closed_form_with_the_sweep(lib):
    C.euler_closed_form(lib)


def test_a_core_still_solves(lib):
    C.core_still_solves(lib)


@pytest.mark.parametrize("scheme", ["mpfa", "tpfa"])
def test_advection_diffusion(lib, scheme):
    C.advdiff(lib, scheme, 4)


def test_deterministic_and_merged_form(lib):
    C.deterministic_and_merged(lib, 6)


def test_errors_and_staleness(lib):
    C.errors(lib)


def test_order_follows_the_flux(lib):
    C.order_follows_the_flux(lib)


def test_nothing_else_moves(lib):
    C.nothing_else_moves(lib, 4)
