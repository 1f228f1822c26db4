"""GPU suite (-m gpu) for the adjoint of the flow solve: the cases of test_flow_adjoint_emulation.py on the gfx950 HIP
library."""
import pytest

import porepy_amd as pa
from tests import _flow_adjoint_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


@pytest.mark.parametrize("name,scheme", C.COMBOS)
def test_split(lib, name, scheme):
    C.split(lib, name, scheme)


@pytest.mark.parametrize("name,scheme", [("cart6x5", "tpfa"), ("tets2", "mpfa")])
def test_split_with_vector_source(lib, name, scheme):
    C.split(lib, name, scheme, vector_source=True)


def test_split_with_amg(lib):
    C.split(lib, "tets3", "mpfa", precond="amg")


@pytest.mark.parametrize("name,scheme", C.COMBOS)
def test_whole_call(lib, name, scheme):
    C.whole(lib, name, scheme)


def test_whole_call_with_vector_source(lib):
    C.whole(lib, "tets2", "tpfa", vector_source=True)


@pytest.mark.parametrize("name,scheme", [("cart6x5", "tpfa"), ("tets2", "mpfa")])
def test_load_combinations(lib, name, scheme):
    C.load_combinations(lib, name, scheme)


def test_one_dimensional_delegate(lib):
    C.one_dimensional_delegate(lib)


def test_determinism_and_maps(lib):
    C.determinism_and_maps(lib)


@pytest.mark.parametrize("name", ["cart6x5", "tets2", "tets3"])
def test_consistent_with_ad_flux_system(lib, name):
    C.consistent_with_ad_flux_system(lib, name, vector_source=name == "tets2")


def _to_device(a):
    import torch

    t = torch.from_numpy(a).cuda()
    torch.cuda.synchronize()
    return t.data_ptr(), t


def test_device_vectors(lib):
    C.device_vectors(lib, _to_device, lambda t: t.cpu().numpy())


def test_chain(lib):
    C.chain(lib)


def test_refusals(lib):
    C.refusals(lib)
