"""CPU suite for the advection-diffusion system and its implicit Euler step (porepy_amd.AdvectionDiffusion) on the
host-emulation build of the same kernels; tests/test_gpu_advdiff.py runs the same cases on the HIP library."""
import pytest

from tests import _advdiff_cases as C
from tests import _parity as P


@pytest.fixture(scope="module")
def lib():
    return P.emulation_library()


def _host(a):
    return a.ctypes.data, a


@pytest.mark.parametrize("name", C.fixture_names())
def test_fixture_parity(lib, name):
    C.fixture_parity(lib, name)


@pytest.mark.parametrize("precond", ["amg", "jacobi"])
@pytest.mark.parametrize("kind", ["tets4", "tets5", "quad", "line"])
def test_five_implicit_euler_steps(lib, kind, precond):
    C.stepping(lib, kind, precond)


def test_device_vectors_and_flux_of_another_handle(lib):
    C.device_vectors_and_foreign_flux(lib, _host, lambda a: a)


@pytest.mark.parametrize("pe", [0.05, 5, 500])
def test_peclet_regimes(lib, pe):
    C.peclet(lib, pe)


def test_failed_amg_step_falls_back_to_jacobi_gmres(lib):
    C.fallback_path(lib)


def test_conservation(lib):
    C.conservation(lib)


def test_update_flux_refreshes_values_only(lib):
    C.update_flux(lib)


def test_limits_no_diffusion_and_no_flux(lib):
    C.limits(lib)


def test_deterministic(lib):
    C.deterministic(lib)


def test_nothing_else_moves(lib):
    C.nothing_else_moves(lib)


def test_errors(lib):
    C.errors(lib)
