"""CPU suite for the adjoint of the saturation step (pfv_transport_adjoint_nl, csrc/sweep.inc: sweep_row_nl_t) on the
host-emulation build of the same kernels; tests/test_gpu_saturation_adjoint.py runs the same cases on the HIP library.
The stand-alone host check of csrc/fluxfn.h's parameter derivatives (tools/fluxfn_params_host_check.cpp) is built with
the address and undefined-behaviour sanitizers and run here."""
import os
import shutil
import subprocess

import pytest

from tests import _parity as P
from tests import _saturation_adjoint_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    return P.emulation_library()


def test_judge_against_differences():
    C.judge_against_differences()


@pytest.mark.skipif(shutil.which("g++") is None, reason="no host compiler")
def test_parameter_derivatives_under_sanitizers(tmp_path):
    """fluxfn_eval_params and f' against central differences of fluxfn_eval (csrc/fluxfn.h), in a stand-alone program
    built with the address and undefined-behaviour sanitizers."""
    exe = str(tmp_path / "fluxfn_params_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "fluxfn_params_host_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    print(out)
    assert "fluxfn params host check: ok" in out


@pytest.mark.parametrize("n", [3, 4])
def test_exact_against_the_judge(lib, n):
    C.exact(lib, n)


def test_table_and_linear(lib):
    C.table_and_linear(lib)


def test_flat_cells(lib):
    C.flat_cells(lib)


def test_line_closed_form(lib):
    C.line_closed_form(lib)


@pytest.mark.parametrize("name", ["cyclic12", "rotation8"])
def test_cyclic_core(lib, name):
    C.cyclic_core(lib, name)


def test_own_forward_differences(lib):
    C.own_forward_differences(lib)


def test_launch_forms_and_determinism(lib):
    C.launch_forms_and_determinism(lib)


def test_observation_forms(lib):
    C.observation_forms(lib)


def test_refusals(lib):
    C.refusals(lib)


def test_handle(lib):
    C.handle(lib)


def test_flow_system_is_untouched(lib):
    C.flow_system_is_untouched(lib)


def test_device_vectors(lib):
    C.device_vectors(lib)
