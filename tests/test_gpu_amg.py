"""GPU suite (-m gpu) for the plain aggregation AMG (PFV_PRECOND_AMG): the cases of test_amg_emulation.py on the gfx950
HIP library, plus what exists only there -- the windowed and fused products (k_spmv_win MODE 4 / 5) on the 24^3 and
30^3 tetrahedral grids under the whole switch matrix, the window fallback, and one grid above kAmgWTopRows where the default
switches alone give gamma = 2 and the fused large-level products."""
import numpy as np
import pytest

import porepy_amd as pa
from tests import _amg_cases as C
from tests.test_amg_emulation import _report

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    return pa._lib.product_library()


def test_device_build(lib):
    assert lib.pfv_is_device_build() == 1


def test_no_hierarchy_and_bad_level(lib):
    from tests.test_amg_emulation import test_no_hierarchy_and_bad_level as body
    body(lib)


def test_tets_two_levels(lib):
    from tests.test_amg_emulation import test_tets_two_levels as body
    body(lib)


def test_tets_coarsest_level_just_under_the_dense_limit(lib):
    from tests.test_amg_emulation import test_tets_coarsest_level_just_under_the_dense_limit as body
    body(lib)


def test_tets_multi_level_small_fused_paths(lib):
    from tests.test_amg_emulation import test_tets_multi_level_small_fused_paths as body
    body(lib)


def test_cartesian_2d(lib):
    from tests.test_amg_emulation import test_cartesian_2d as body
    body(lib)


def test_heterogeneous_cartesian_3d(lib):
    from tests.test_amg_emulation import test_heterogeneous_cartesian_3d as body
    body(lib)


@pytest.mark.parametrize("dim", [2, 3])
def test_block_systems(lib, dim):
    from tests.test_amg_emulation import test_block_systems as body
    body(lib, dim)


def test_user_csr_unsorted_singleton_and_hub(lib):
    from tests.test_amg_emulation import test_user_csr_unsorted_singleton_and_hub as body
    body(lib)


def test_user_csr_without_locality(lib):
    from tests.test_amg_emulation import test_user_csr_without_locality as body
    body(lib)


def test_jacobi_fallback_on_a_stalled_coarsest_level(lib):
    from tests.test_amg_emulation import test_jacobi_fallback_on_a_stalled_coarsest_level as body
    body(lib)


def test_leading_block(lib):
    C.leading_block(lib)


def test_state_sequence(lib):
    for tag, out in C.state_sequence(lib, 10):
        _report("state / " + tag, out)


def test_matching_switch_change_rematches(lib):
    assert C.matching_switch_change_rematches(lib, 8) >= 3


def test_different_pattern_with_equal_sizes_rebuilds_the_maps(lib):
    C.different_pattern_same_sizes(lib)


def test_mutations_of_the_reference_are_detected(lib):
    assert C.mutations(lib, 10)


def test_switch_matrix_24_cubed(lib):
    """The 24^3 grid of test_amg_fused_cycle_is_the_same_operator.  The read-out shows that only its level 0 has an SpMV
    window: the first coarse level (8 872 rows) stays below the 200 000 entries from which amg_setup builds one, so its
    fused products are the plain-CSR forms (k_amg_spmv MODE 4 / 5).  test_switch_matrix_windowed_coarse_level is the
    grid on which the windowed forms run."""
    def expect(H):
        assert len(H) >= 4 and H[0]["window"], [(h["n"], h["window"]) for h in H]
    res = C.switch_matrix(lambda: C.FlowSystem(lib, C.tet_grid(24, 0.012), seed=4), lib, expect_default=expect)
    for name, out in res.items():
        _report("switches tets 24^3 / " + name, out)
    assert "second_visit_fused" in res["gamma=2"]["H"][0]["path"]
    assert "fused_product" in res["fuse_rows=0,gamma=2"]["H"][1]["path"]


def test_switch_matrix_windowed_coarse_level(lib):
    """30^3 perturbed tetrahedra: level 0 and the first coarse level have SpMV windows, so the variants reach the
    windowed forms of every product (k_spmv_win MODE 0 / 1 / 4 / 5)."""
    def expect(H):
        assert len(H) >= 4 and H[0]["window"] and H[1]["window"], [(h["n"], h["op"].nnz, h["window"]) for h in H]
        assert "fused_product" in H[1]["path"]  # (a windowed level never takes the small-level launches)
    res = C.switch_matrix(lambda: C.FlowSystem(lib, C.tet_grid(30, 0.01), seed=4), lib, expect_default=expect)
    for name, out in res.items():
        _report("switches tets 30^3 / " + name, out)
    assert "second_visit_fused" in res["gamma=2"]["H"][0]["path"]


def test_switch_matrix_block(lib):
    res = C.switch_matrix(lambda: C.MechSystem(lib, C.tet_grid(8)), lib)
    assert res["default"]["levels"] >= 3
    for name, out in res.items():
        _report("switches mpsa 8^3 / " + name, out)


def test_large_grid_default_switches(lib):
    """48^3 tetrahedra (663 552 cells >= kAmgWTopRows): gamma = 2 and the fused large-level products by the defaults
    alone.  The cycle is judged against the float64 reference (baseline: float64 against float64 with reversed rows)."""
    S = C.FlowSystem(lib, C.tet_grid(48, 0.005), seed=8)
    S.ctx.amg_setup(0)
    H = C.read_hierarchy(S.ctx)
    assert H[0]["n"] >= H[0]["w_top_rows"] and H[0]["gamma"] == 2 and H[0]["fuse_cycle"]
    assert "second_visit_fused" in H[0]["path"] and {"fused_product", "visited_twice"} <= H[1]["path"]
    assert H[0]["window"] and H[1]["window"]
    out = C.check_setup(H)
    out["cycle"] = C.check_cycle(S.ctx, lib, H, seed=5, dtype=np.float64)
    out["paths"] = C.paths(H)
    _report("tets 48^3 (float64 reference)", out)
