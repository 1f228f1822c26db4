"""CPU suite for the sorbing transport step (pfv_transport_advance_sorb, csrc/sweep.inc: sweep_row_sorb) on the
host-emulation build of the same kernels; tests/test_gpu_sorb.py runs the same cases on the HIP library."""
import os
import shutil
import subprocess

import pytest

from tests import _parity as P
from tests import _sorb_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return P.emulation_library()


def test_judges_agree():
    C.judges_agree()


@pytest.mark.parametrize("name", list(C.ISOTHERMS))
@pytest.mark.parametrize("n", [3, 4])
def test_exact_on_an_acyclic_flux(lib, n, name):
    C.exact(lib, n, name)


@pytest.mark.parametrize("name", C.NONLINEAR)
def test_line_against_its_recursion(lib, name):
    C.line_case(lib, name)


def test_linear_is_the_linear_step_bit_for_bit(lib):
    C.linear_is_the_linear_step(lib)


@pytest.mark.parametrize("k,solo", [(5, (0, 1, 2, 3, 4)), (64, (63, 0))])
def test_components_do_not_see_each_other(lib, k, solo):
    C.independent(lib, k, solo)


@pytest.mark.parametrize("which", ["cyclic12", "rotation8"])
def test_cyclic_core_converges(lib, which):
    C.core_converges(lib, which)


def test_deterministic_and_merged(lib):
    C.deterministic_and_merged(lib)


def test_mass(lib):
    C.mass(lib)


def test_no_non_negative_root(lib):
    C.no_root(lib)


def test_errors(lib):
    C.errors(lib)


def test_lifetime(lib):
    C.lifetime(lib)


def test_flow_system_is_untouched(lib):
    C.flow_system_is_untouched(lib)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_host_code_under_sanitizers(tmp_path):
    """The check and the evaluation of the isotherms (csrc/isotherm.h), in a stand-alone program built with the address
    and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "isotherm_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "isotherm_host_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "isotherm host check: ok" in out
