"""CPU suite for the reactive transport step (pfv_transport_advance_react, csrc/sweep.inc: sweep_row_react) on the
host-emulation build of the same kernels; tests/test_gpu_react.py runs the same cases on the HIP library."""
import os
import shutil
import subprocess

import pytest

from tests import _parity as P
from tests import _react_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return P.emulation_library()


@pytest.mark.parametrize("n,k", [(3, 4), (4, 4), (3, 3), (4, 3), (3, 8), (4, 8)])
def test_exact_against_the_whole_system(lib, n, k):
    C.exact(lib, n, k)


def test_reduces_to_independent_components(lib):
    C.reduces_to_components(lib)


def test_chain_on_the_line_closed_form(lib):
    C.closed_form(lib)


def test_immobile_partner(lib):
    C.immobile_partner(lib)


def test_conservation(lib):
    C.conservation(lib)


def test_positivity(lib):
    C.positivity(lib)


def test_launch_forms_and_determinism(lib):
    C.launch_forms(lib)


@pytest.mark.parametrize("which", ["cyclic12", "rotation8", "cyclic12-k3"])
def test_cyclic_core(lib, which):
    C.core_case(lib, which)


def test_refusals(lib):
    C.refusals(lib)


def test_handle(lib):
    C.handle(lib)


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_host_code_under_sanitizers(tmp_path):
    """The check of the rate matrix and the mobilities (csrc/react.h), in a stand-alone program built with the address
    and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "react_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "react_host_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    assert "react host check: ok" in out
