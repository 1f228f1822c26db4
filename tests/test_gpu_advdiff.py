"""GPU suite (-m gpu) for the advection-diffusion system and its implicit Euler step: the cases of
test_advdiff_emulation.py on the gfx950 HIP library, every vector of the device-pointer case in device memory."""
import pytest

import porepy_amd as pa
from tests import _advdiff_cases as C

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


@pytest.mark.parametrize("precond", ["amg", "jacobi"])
@pytest.mark.parametrize("kind", ["tets4", "tets5", "quad", "line"])
def test_five_implicit_euler_steps(lib, kind, precond):
    C.stepping(lib, kind, precond)


def test_device_vectors_and_flux_of_another_handle(lib):
    C.device_vectors_and_foreign_flux(lib, _to_device, _to_host)


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
