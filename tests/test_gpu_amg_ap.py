"""GPU suite (-m gpu) for the finest level's post-smoothing through AP = A_s P (PFV_AMG_POST_AP): the cases of
test_amg_ap_emulation.py on the gfx950 HIP library, plus a grid whose level 0 has an SpMV window (its residual product
is the windowed kernel; the new launch gathers from the coarse vector without one)."""
import pytest

import porepy_amd as pa
from tests import _amg_ap_cases as A
from tests import _amg_cases as C

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


def test_tets_w_cycle_folds_the_second_visit(lib):
    A.tets_w_cycle(lib)


def test_tets_v_cycle(lib):
    A.tets_v_cycle(lib)


def test_cartesian_2d_rows_not_a_multiple_of_64(lib):
    A.cartesian_2d(lib)


def test_user_csr_without_locality(lib):
    A.without_locality(lib)


def test_stalled_coarsest_level(lib):
    A.stalled(lib)


def test_rows_longer_than_the_ranked_ones(lib):
    A.long_rows(lib)


def test_block_system_keeps_the_two_launches(lib):
    A.block_system(lib)


def test_fp64_values_keep_the_two_launches(lib):
    A.fp64_fallback(lib)


def test_same_bits_from_two_setups_and_two_applies(lib):
    assert A.determinism(lib)


def test_solve_on_against_off(lib):
    A.solve_on_against_off(lib, C.tet_grid(8))


def test_windowed_level_0(lib):
    def expect(H):
        assert H[0]["window"] and len(H) >= 3
    A.on_against_off(lambda: C.FlowSystem(lib, C.tet_grid(16, 0.015), seed=4), lib, {"PFV_AMG_GAMMA": "2"}, expect=expect)
