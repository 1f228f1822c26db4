"""GPU suite (-m gpu) for the exact permeability gradient of the MPFA flow solve: the cases of
test_mpfa_adjoint_emulation.py on the gfx950 HIP library."""
import os

import numpy as np
import pytest

import porepy_amd as pa
from tests import _mpfa_adjoint_cases as C

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "mpfa_adjoint", "two_point_permeability.npz")


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


@pytest.mark.parametrize("vector_source", [False, True])
@pytest.mark.parametrize("name", C.MPFA_GRIDS)
def test_library_against_judge(lib, name, vector_source):
    C.library_against_judge(lib, name, vector_source)


def test_k_orthogonal(lib):
    C.k_orthogonal(lib)


def test_it_matters(lib):
    C.it_matters(lib, np.load(GOLDEN)["mi355x"])


def test_chain(lib):
    C.chain(lib)


def test_determinism_and_map(lib):
    C.determinism_and_map(lib)


def test_tpfa_and_delegate(lib):
    C.tpfa_and_delegate(lib)


def _to_device(a):
    import torch

    t = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    return t.data_ptr(), t


def test_device_vectors(lib):
    C.device_vectors(lib, _to_device, lambda t: t.cpu().numpy())


def _alloc(n):
    import torch

    t = torch.zeros(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return t.data_ptr(), t


def test_refusals(lib):
    C.refusals(lib, _alloc)


def test_region_too_large(lib):
    C.region_too_large(lib)
