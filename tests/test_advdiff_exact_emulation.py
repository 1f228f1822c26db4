"""CPU suite for the exact conductivity gradient of the advection-diffusion adjoint (pfv_advdiff_adjoint_exact,
csrc/mpfa_adjoint.inc: adj_batch_body) on the host-emulation build of the same kernels; tests/test_gpu_advdiff_exact.py
runs the same cases on the HIP library."""
import pytest

from tests import _advdiff_adjoint_cases as AA
from tests import _advdiff_exact_cases as C
from tests import _parity as P


@pytest.fixture(scope="module")
def lib():
    return P.emulation_library()


@pytest.mark.parametrize("kind,stride,entry", [("tets3", 7, e) for e in C.ALL_ENTRIES] +
                         [("cart6x5", 1, e) for e in C.PLANE_ENTRIES])
def test_judge_against_differences(kind, stride, entry):
    C.judge_against_differences(kind, stride=stride, entries=(entry,))


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


def test_device_vectors(lib):
    C.device_vectors(lib)


def test_refusals(lib):
    C.refusals(lib)


def test_region_too_large(lib):
    C.region_too_large(lib)
