"""The sub-cell topology rebuild on the HIP library (MI355X): the node-cooperative construction against the reference
construction (PFV_TOPO_LEGACY=1) and a numpy construction, array by array and bit for bit (tests/_topology_cases.py);
tests/test_topology_rebuild_emulation.py runs the same cases on the host-emulation build."""
import pytest

import porepy_amd as pa
from tests import _topology_cases as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


@pytest.mark.parametrize("name", list(T.REGULAR))
def test_rebuild_three_ways(lib, name):
    T.check_case(lib, name)


def test_fan_of_256_is_unsupported_on_both_paths(lib):
    T.check_error(lib, T.fan_2d(256), 5, "more than 255 faces or cells meet in one node")


def test_pyramid_apex_is_a_cell_shape_error_on_both_paths(lib):
    T.check_error(lib, T.pyramid(), 2, "exactly nd faces meeting in one of its nodes")


def test_rebuild_twice_then_another_grid(lib):
    T.check_rebuild_sequence(lib)


def test_matrices_bit_identical_between_the_paths(lib):
    T.check_matrices_bit_identical(lib)
