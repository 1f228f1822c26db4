"""CPU suite for the saturation step with phase-carried components (pfv_transport_advance_nl_multi, csrc/sweep.inc:
sweep_row_nlc) on the host-emulation build of the same kernels; tests/test_gpu_satcomp.py runs the same cases on the HIP
library."""
import pytest

from tests import _parity as P
from tests import _satcomp_cases as C


@pytest.fixture(scope="module")
def lib():
    return P.emulation_library()


def test_judges_agree_on_the_line():
    C.judges_agree_on_the_line()


@pytest.mark.parametrize("k", [1, 3, 4, 5])
@pytest.mark.parametrize("n,kind", [(3, "corey"), (3, "table"), (4, "corey"), (4, "table")])
def test_against_the_judge(lib, n, kind, k):
    C.against_judge(lib, n, kind, k)


@pytest.mark.parametrize("sorb", [False, True])
@pytest.mark.parametrize("n_w,n_n,wells", [(2.0, 2.0, False), (3.0, 1.5, False), (2.0, 2.0, True), (3.0, 1.5, True)])
def test_line_against_its_recursion(lib, n_w, n_n, wells, sorb):
    C.line_case(lib, n_w, n_n, wells, sorb)


def test_line_with_64_components(lib):
    C.line_k64(lib)


@pytest.mark.parametrize("where", ["tets4", "line"])
def test_water_marking_invariant(lib, where):
    C.water_marking(lib, where)


def test_reduces_to_the_linear_components_step(lib):
    C.reduces_to_linear_components(lib)


@pytest.mark.parametrize("which", ["tets4", "cyclic12", "rotation8"])
def test_saturation_unchanged(lib, which):
    C.saturation_unchanged(lib, which)


def test_launch_forms(lib):
    C.launch_forms(lib)


@pytest.mark.parametrize("which", ["cyclic12", "rotation8", "cyclic12-k64"])
def test_core_iterates_jointly(lib, which):
    C.core_case(lib, which)


def test_refused_step(lib):
    C.refused_step(lib)


def test_errors(lib):
    C.errors(lib)


def test_handle(lib):
    C.handle(lib)


def test_flow_system_is_untouched(lib):
    C.flow_system_is_untouched(lib)
