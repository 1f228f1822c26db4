"""GPU suite (-m gpu) for the exact conductivity gradient of the advection-diffusion adjoint: the cases of
test_advdiff_exact_emulation.py on the gfx950 HIP library."""
import pytest

import porepy_amd as pa
from tests import _advdiff_adjoint_cases as AA
from tests import _advdiff_exact_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


@pytest.mark.parametrize("regime", list(AA.REGIMES))
@pytest.mark.parametrize("kind", C.MPFA_GRIDS)
def test_library_against_judge(lib, kind, regime):
    C.library_against_judge(lib, kind, regime)


@pytest.mark.parametrize("regime", list(AA.REGIMES))
@pytest.mark.parametrize("kind", C.MPFA_GRIDS)
def test_whole_call(lib, kind, regime):
    C.whole_call(lib, kind, regime)


def test_library_against_own_differences(lib):
    C.library_against_own_differences(lib)


def test_it_matters(lib):
    C.it_matters(lib)


@pytest.mark.parametrize("kind", ["cart6x5", "tets2"])
def test_batch_invariance(lib, kind):
    C.batch_invariance(lib, kind)


def test_other_outputs_unchanged(lib):
    C.other_outputs_unchanged(lib)


def test_k_orthogonal(lib):
    C.k_orthogonal(lib)


def test_tpfa_and_delegate(lib):
    C.tpfa_and_delegate(lib)


def _to_device(a):
    import torch

    t = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    return t.data_ptr(), t


def test_device_vectors(lib):
    C.device_vectors(lib, _to_device, lambda t: t.cpu().numpy())


def test_refusals(lib):
    C.refusals(lib)


def test_region_too_large(lib):
    C.region_too_large(lib)
