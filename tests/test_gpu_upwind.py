"""GPU suite (-m gpu) for the upwind discretization and the transport step: the cases of test_upwind_emulation.py on
the gfx950 HIP library, plus the larger grids."""
import pytest

import porepy_amd as pa
from tests import _upwind_cases as C

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


@pytest.mark.parametrize("name", C.fixture_names())
def test_fixture_parity(lib, name):
    C.fixture_parity(lib, name)


def test_nan_flux_takes_the_negative_branch(lib):
    C.nan_goes_to_the_negative_branch(lib)


@pytest.mark.parametrize("n", [12, 32])
def test_random_signs_against_numpy_restatement(lib, n):
    C.random_signs(lib, n)


def test_implicit_euler_closed_form(lib):
    C.euler_closed_form(lib)


def test_conservation_and_bounds(lib):
    C.conservation_and_bounds(lib, 6)


@pytest.mark.parametrize("scheme", ["mpfa", "tpfa"])
def test_resident_pipeline(lib, scheme):
    C.resident_pipeline(lib, 8, _to_device, _to_host, scheme)


def test_advection_diffusion_through_device_csr(lib):
    C.advection_diffusion(lib, 6)


def test_deterministic(lib):
    C.deterministic(lib, 6)


def test_nothing_else_moves(lib):
    C.nothing_else_moves(lib, 6)


def test_errors(lib):
    C.errors(lib)


def test_injection_from_rest_with_the_default_method(lib):
    C.injection_from_rest(lib, 6)


@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("scheme,dim", [("mpfa", 3), ("mpfa", 2), ("tpfa", 3)])
def test_face_flux_with_vector_source(lib, scheme, dim, implicit):
    C.face_flux_with_vector_source(lib, scheme, dim, implicit)


def test_stale_transport_system_is_not_solved(lib):
    C.stale_system_is_not_solved(lib)
