"""CPU suite for the adjoint of the flow solve (pfv_flow_adjoint, csrc/flow_adjoint.inc) on the host-emulation build of
the same kernels; tests/test_gpu_flow_adjoint.py runs the same cases on the HIP library."""
import pytest

from tests import _flow_adjoint_cases as C
from tests import _parity as P


@pytest.fixture(scope="module")
def lib():
    return P.emulation_library()


def test_judge_against_differences():
    C.judge_against_differences()


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


def test_device_vectors(lib):
    C.device_vectors(lib)


def test_chain(lib):
    C.chain(lib)


def test_refusals(lib):
    C.refusals(lib)
