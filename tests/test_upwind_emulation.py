"""CPU suite for the upwind discretization and the transport step (porepy_amd.Upwind) on the host-emulation build of
the same kernels; tests/test_gpu_upwind.py runs the same cases on the HIP library."""
import pytest

from tests import _parity as P
from tests import _upwind_cases as C


@pytest.fixture(scope="module")
def lib():
    return P.emulation_library()


def _host(a):
    return a.ctypes.data, a


@pytest.mark.parametrize("name", C.fixture_names())
def test_fixture_parity(lib, name):
    C.fixture_parity(lib, name)


def test_nan_flux_takes_the_negative_branch(lib):
    C.nan_goes_to_the_negative_branch(lib)


def test_random_signs_against_numpy_restatement(lib):
    C.random_signs(lib, 12)


def test_implicit_euler_closed_form(lib):
    C.euler_closed_form(lib)


def test_conservation_and_bounds(lib):
    C.conservation_and_bounds(lib, 4)


@pytest.mark.parametrize("scheme", ["mpfa", "tpfa"])
def test_resident_pipeline(lib, scheme):
    C.resident_pipeline(lib, 5, _host, lambda a: a, scheme)


def test_advection_diffusion_through_device_csr(lib):
    C.advection_diffusion(lib, 4)


def test_deterministic(lib):
    C.deterministic(lib, 4)


def test_nothing_else_moves(lib):
    C.nothing_else_moves(lib, 4)


def test_errors(lib):
    C.errors(lib)


def test_injection_from_rest_with_the_default_method(lib):
    C.injection_from_rest(lib, 4)


@pytest.mark.parametrize("implicit", [False, True])
@pytest.mark.parametrize("scheme,dim", [("mpfa", 3), ("mpfa", 2), ("tpfa", 3)])
def test_face_flux_with_vector_source(lib, scheme, dim, implicit):
    C.face_flux_with_vector_source(lib, scheme, dim, implicit)


def test_stale_transport_system_is_not_solved(lib):
    C.stale_system_is_not_solved(lib)
