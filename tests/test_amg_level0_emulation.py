"""CPU suite for level 0 of the AMG cycle on its AP path (PFV_AMG_L0_RESIDUAL, PFV_AMG_KRYLOV_PRESMOOTH) on the
host-emulation build of the same sources: the cases of tests/_amg_level0_cases.py.  tests/test_gpu_amg_level0.py runs
them on the HIP library, where levels have windows."""
import pytest

from tests import _amg_cases as C
from tests import _amg_level0_cases as L0
from tests import _parity as P


@pytest.fixture(scope="module")
def lib():
    return P.emulation_library()


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


def test_presmoothing_in_the_krylov_updates_keeps_the_bits(lib):
    assert L0.presmoothing_in_the_krylov_updates(lib, C.tet_grid(8))


def test_solve_all_on_against_all_off(lib):
    assert L0.solve_all_on_against_all_off(lib, C.tet_grid(8))
