"""CPU suite for the adjoint of the saturation step with phase-carried components (pfv_transport_adjoint_nl_multi,
csrc/sweep.inc: sweep_row_nlc_t) on the host-emulation build of the same kernels;
tests/test_gpu_satcomp_adjoint.py runs the same cases on the HIP library."""
import pytest

from tests import _parity as P
from tests import _satcomp_adjoint_cases as C


@pytest.fixture(scope="module")
def lib():
    return P.emulation_library()


def test_judge_against_differences():
    C.judge_against_differences()


@pytest.mark.parametrize("k", [1, 3, 5])
@pytest.mark.parametrize("n", [3, 4])
def test_exact_against_the_judge(lib, n, k):
    C.exact(lib, n, k)


def test_no_component_loads(lib):
    C.no_component_loads(lib)


def test_linear_constant_saturation(lib):
    C.linear_constant_saturation(lib)


def test_table(lib):
    C.table(lib)


@pytest.mark.parametrize("k", [2, 64])
def test_line(lib, k):
    C.line(lib, k)


@pytest.mark.parametrize("name", ["cyclic12", "rotation8"])
def test_cyclic_core(lib, name):
    C.cyclic_core(lib, name)


def test_own_forward_differences(lib):
    C.own_forward_differences(lib)


def test_launch_forms_and_determinism(lib):
    C.launch_forms_and_determinism(lib)


def test_observation_forms(lib):
    C.observation_forms(lib)


def test_device_vectors(lib):
    C.device_vectors(lib)


def test_refusals(lib):
    C.refusals(lib)


def test_handle(lib):
    C.handle(lib)


def test_flow_system_is_untouched(lib):
    C.flow_system_is_untouched(lib)
