"""GPU suite (-m gpu) for level 0 of the AMG cycle on its AP path: the cases of test_amg_level0_emulation.py on the gfx950
HIP library -- where the filtered level 0 has SpMV windows, so the residual form of the windowed product
(k_spmv_win MODE 6) and k_amg_post_ap run --, plus a grid with several hundred row blocks."""
import pytest

import porepy_amd as pa
from tests import _amg_cases as C
from tests import _amg_level0_cases as L0

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


def test_tets_w_cycle_folds_the_second_visit(lib):
    L0.tets_w_cycle(lib)


def test_tets_v_cycle(lib):
    L0.tets_v_cycle(lib)


def test_cartesian_2d_last_window_short(lib):
    L0.cartesian_last_window_short(lib)


def test_cartesian_2d_last_group_of_three_windows(lib):
    L0.cartesian_last_group_of_three(lib)


def test_hub_row_spanning_chunks(lib):
    L0.long_rows(lib)


def test_windowed_level_0_many_blocks(lib):
    on, _ = L0.windowed_many_blocks(lib)
    assert on["H"][0]["window"]


def test_user_csr_without_locality(lib):
    L0.without_locality(lib)


def test_stalled_coarsest_level(lib):
    L0.stalled(lib)


def test_block_system_takes_none_of_it(lib):
    L0.block_system(lib)


def test_fp64_values_take_none_of_it(lib):
    L0.fp64_fallback(lib)


def test_same_bits_from_two_setups_and_two_applies(lib):
    assert L0.determinism(lib)


def test_residual_form_alone_keeps_the_bits_of_the_coarse_rhs(lib):
    assert L0.residual_form_keeps_the_coarse_rhs(lib)


def test_residual_form_alone_keeps_the_bits_on_many_blocks(lib):
    assert L0.residual_form_keeps_the_coarse_rhs(lib, lambda: C.FlowSystem(lib, C.tet_grid(16, 0.015), seed=4))


def test_presmoothing_in_the_krylov_updates_keeps_the_bits(lib):
    assert L0.presmoothing_in_the_krylov_updates(lib, C.tet_grid(8))


def test_solve_all_on_against_all_off(lib):
    assert L0.solve_all_on_against_all_off(lib, C.tet_grid(8))
