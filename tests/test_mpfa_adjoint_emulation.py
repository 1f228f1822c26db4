"""CPU suite for the exact permeability gradient of the MPFA flow solve (pfv_flow_adjoint_exact, csrc/mpfa_adjoint.inc)
on the host-emulation build of the same kernels; tests/test_gpu_mpfa_adjoint.py runs the same cases on the HIP library."""
import os

import numpy as np
import pytest

from tests import _mpfa_adjoint_cases as C
from tests import _parity as P

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "mpfa_adjoint", "two_point_permeability.npz")


@pytest.fixture(scope="module")
def lib():
    return P.emulation_library()


@pytest.mark.parametrize("entry", C.ALL_ENTRIES)
@pytest.mark.parametrize("name,stride,vector_source", [("tets3", 7, True), ("cart6x5", 1, False)])
def test_judge_against_differences(name, stride, vector_source, entry):
    C.judge_against_differences(name, stride=stride, vector_source=vector_source, entries=(entry,))


@pytest.mark.parametrize("vector_source", [False, True])
@pytest.mark.parametrize("name", C.MPFA_GRIDS)
def test_library_against_judge(lib, name, vector_source):
    C.library_against_judge(lib, name, vector_source)


def test_k_orthogonal(lib):
    C.k_orthogonal(lib)


def test_it_matters(lib):
    C.it_matters(lib, np.load(GOLDEN)["emulation"])


def test_chain(lib):
    C.chain(lib)


def test_determinism_and_map(lib):
    C.determinism_and_map(lib)


def test_tpfa_and_delegate(lib):
    C.tpfa_and_delegate(lib)


def test_device_vectors(lib):
    C.device_vectors(lib)


def test_refusals(lib):
    C.refusals(lib)


def test_region_too_large(lib):
    C.region_too_large(lib)
