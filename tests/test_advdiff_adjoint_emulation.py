"""CPU suite for the adjoint of the advection-diffusion step (pfv_advdiff_adjoint, csrc/advdiff_adjoint.inc) on the
host-emulation build of the same kernels; tests/test_gpu_advdiff_adjoint.py runs the same cases on the HIP library."""
import pytest

from tests import _advdiff_adjoint_cases as C
from tests import _parity as P


@pytest.fixture(scope="module")
def lib():
    return P.emulation_library()


def test_judge_against_differences():
    C.judge_against_differences()


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


def test_device_vectors(lib):
    C.device_vectors(lib)


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
