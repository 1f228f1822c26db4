"""CPU suite for the saturation step (pfv_transport_advance_nl, csrc/sweep.inc: sweep_row_nl) on the host-emulation
build of the same kernels; tests/test_gpu_saturation.py runs the same cases on the HIP library."""
import os
import shutil
import subprocess

import pytest

from tests import _parity as P
from tests import _saturation_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return P.emulation_library()


def test_judges_agree_on_the_line():
    C.judges_agree_on_the_line()


@pytest.mark.parametrize("n,kind", [(3, "corey"), (3, "table"), (4, "corey"), (4, "table")])
def test_exact_against_global_newton(lib, n, kind):
    C.exact(lib, n, kind)


@pytest.mark.parametrize("n_w,n_n,wells", [(2.0, 2.0, False), (3.0, 1.5, False), (2.0, 2.0, True), (3.0, 1.5, True)])
def test_line_against_its_recursion(lib, n_w, n_n, wells):
    C.line_case(lib, n_w, n_n, wells)


def test_linear_kind_is_the_linear_step(lib):
    C.linear_kind_is_the_linear_step(lib)


@pytest.mark.parametrize("which", ["cyclic12", "rotation8"])
def test_core_converges(lib, which):
    C.core_converges(lib, which)


def test_deterministic_and_merged_form(lib):
    C.deterministic_and_merged(lib)


def test_leaves_the_interval(lib):
    C.leaves_the_interval(lib)


def test_errors(lib):
    C.errors(lib)


def test_lifetime(lib):
    C.lifetime(lib)


def test_flow_system_is_untouched(lib):
    C.flow_system_is_untouched(lib)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_host_code_under_sanitizers(tmp_path):
    """The parameter check and the host-side evaluation of the flux functions (csrc/fluxfn.h), in a stand-alone program
    built with the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "fluxfn_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "fluxfn_host_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "fluxfn host check: ok" in out
