"""GPU suite (-m gpu) for the adjoint of the advection-diffusion step: the cases of test_advdiff_adjoint_emulation.py on
the gfx950 HIP library."""
import pytest

import porepy_amd as pa
from tests import _advdiff_adjoint_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


@pytest.mark.parametrize("regime", list(C.REGIMES))
@pytest.mark.parametrize("kind,scheme", C.COMBOS)
def test_split(lib, kind, scheme, regime):
    C.split(lib, kind, scheme, regime)


@pytest.mark.parametrize("regime", list(C.REGIMES))
@pytest.mark.parametrize("kind,scheme", [("quad", "tpfa"), ("tets3", "mpfa")])
def test_split_with_amg(lib, kind, scheme, regime):
    C.split(lib, kind, scheme, regime, precond="amg")


@pytest.mark.parametrize("regime", list(C.REGIMES))
@pytest.mark.parametrize("kind,scheme", C.COMBOS)
def test_whole_call(lib, kind, scheme, regime):
    C.whole(lib, kind, scheme, regime)


@pytest.mark.parametrize("kind,scheme", [("quad", "tpfa"), ("tets2", "mpfa")])
def test_observations_and_wants(lib, kind, scheme):
    C.observations_and_wants(lib, kind, scheme)


def test_repeat_and_maps(lib):
    C.repeat_and_maps(lib)


def _to_device(a):
    import torch

    t = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    return t.data_ptr(), t


def test_device_vectors(lib):
    C.device_vectors(lib, _to_device, lambda t: t.cpu().numpy())


def test_fallback_path(lib):
    C.fallback_path(lib)


@pytest.mark.parametrize("kind", ["quad", "tets2"])
def test_gmres_retry_path(lib, kind):
    C.gmres_retry_path(lib, kind)


@pytest.mark.parametrize("kind", ["quad", "tets2", "tets3"])
def test_mpfa_consistency(lib, kind):
    C.mpfa_consistency(lib, kind)


def test_chain(lib):
    C.chain(lib)


@pytest.mark.parametrize("kind,scheme", [("line", "tpfa"), ("tets2", "mpfa")])
def test_return_states(lib, kind, scheme):
    C.return_states(lib, kind, scheme)


def test_refusals(lib):
    C.refusals(lib)


def test_handle_afterwards(lib):
    C.handle_afterwards(lib)
