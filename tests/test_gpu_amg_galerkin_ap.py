"""GPU suite (-m gpu) for the first coarse operator formed from AP = A_s P on kept aggregate maps (PFV_AMG_GALERKIN_AP):
the cases of test_amg_galerkin_ap_emulation.py on the gfx950 HIP library, plus a grid whose level 0 has an SpMV window
(the condition under which the large systems build AP without PFV_AMG_FUSE_ROWS=0)."""
import pytest

import porepy_amd as pa
from tests import _amg_cases as C
from tests import _amg_galerkin_ap_cases as G

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


def test_tets_w_cycle(lib):
    G.tets(lib, 2)


def test_tets_v_cycle(lib):
    G.tets(lib, 1)


def test_cartesian_3d_heterogeneous(lib):
    G.cartesian_3d(lib)


def test_rows_longer_than_the_ranked_ones(lib):
    G.long_rows(lib)


def test_coarse_rows_of_the_64_lane_group(lib):
    G.wide_coarse_rows(lib)


def test_aggregate_with_more_members_than_the_batched_gather_takes(lib):
    G.many_members(lib)


def test_user_csr_without_locality(lib):
    G.without_locality(lib)


def test_block_system_takes_the_passes(lib):
    G.fallback_block_system(lib)


def test_fp64_values_take_the_passes(lib):
    out = G.fallback_switch(lib, {"PFV_AMG_FP32": "0"})
    assert not any(h["fp32"] for h in out["H"])


def test_without_ap_the_passes(lib):
    G.fallback_switch(lib, {"PFV_AMG_POST_AP": "0"})


def test_cold_setup_and_matching_switch_change_take_the_passes(lib):
    G.fallback_cold_and_switch_change(lib)


def test_different_pattern_of_equal_sizes_takes_the_passes(lib):
    G.fallback_different_pattern(lib)


def test_state_sequence(lib):
    G.state_sequence(lib)


def test_same_bits_from_two_kept_setups(lib):
    assert G.determinism(lib)


def test_solve_route_against_passes(lib):
    G.solve_route_against_passes(lib, C.tet_grid(8))


def test_windowed_level_0(lib):
    def expect(H):
        assert H[0]["window"] and len(H) >= 3
    G.case(lambda: C.FlowSystem(lib, C.tet_grid(16, 0.015), seed=4), G.move_flow, lib, {"PFV_AMG_GAMMA": "2"}, expect)
