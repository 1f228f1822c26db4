"""CPU suite for the plain aggregation AMG (PFV_PRECOND_AMG) on the host-emulation build of the same sources: setup
identities, the cycle against a plain longdouble reference and the state a re-setup keeps, all from the read-out of
Context.amg_level.  tests/test_gpu_amg.py runs the same cases on the HIP library (plus the windowed / fused products,
which exist only there)."""
import numpy as np
import pytest

from tests import _amg_cases as C
from tests import _parity as P


@pytest.fixture(scope="module")
def lib():
    return P.emulation_library()


def _report(name, out):
    cyc = out["cycle"]
    print(f"amg case {name}: rows {out['rows']} paths {out['paths']} cycle baseline {cyc['baseline']:.2e} "
          f"bound {cyc['bound']:.2e} error {cyc['error']:.2e} galerkin {[tuple(f'{v:.1e}' for v in g) for g in out['galerkin']]} "
          f"filter {out['filter']} dense {out.get('dense')}")


def test_no_hierarchy_and_bad_level(lib):
    S = C.UserSystem(lib, C.graph_matrix(300, np.random.default_rng(0)))
    info = np.zeros(24, dtype=np.int64)
    none = [None] * 15
    assert lib.pfv_amg_level(S.ctx._h, 0, info.ctypes.data_as(C._lib._lp), *none) == 4  # no hierarchy yet
    S.ctx.amg_setup(0)
    lev = S.ctx.amg_level(0)
    assert lib.pfv_amg_level(S.ctx._h, lev["levels"], info.ctypes.data_as(C._lib._lp), *none) == 4
    assert lib.pfv_amg_level(S.ctx._h, -1, info.ctypes.data_as(C._lib._lp), *none) == 4
    assert lib.pfv_amg_level(S.ctx._h, 0, None, *none) == 4


def test_tets_two_levels(lib):
    def expect(H):
        assert len(H) == 2 and H[0]["n"] % 64 != 0 and H[1]["dense_ok"]
    _report("tets 5^3", C.run_case(C.FlowSystem(lib, C.tet_grid(5)), lib, expect=expect))


def test_tets_coarsest_level_just_under_the_dense_limit(lib):
    def expect(H):
        assert 0.6 * H[0]["dense_max"] <= H[-1]["n"] <= H[0]["dense_max"] and H[-1]["dense_ok"], H[-1]["n"]
        assert H[0]["n"] % 64 != 0
    out = C.run_case(C.FlowSystem(lib, C.tet_grid(11)), lib, env={"PFV_AMG_COARSE_TARGET": "1024"}, expect=expect)
    _report("tets 11^3, coarse target 1024", out)


def test_tets_multi_level_small_fused_paths(lib):
    def expect(H):
        assert len(H) >= 3 and H[0]["n"] % 256 != 0
        assert "restrict_residual" in H[0]["path"] and "prolong_smooth" in H[1]["path"]
    _report("tets 9^3", C.run_case(C.FlowSystem(lib, C.tet_grid(9)), lib, expect=expect))


def test_cartesian_2d(lib):
    _report("cart 40x30", C.run_case(C.FlowSystem(lib, C.cart_grid([40, 30])), lib, ))


def test_heterogeneous_cartesian_3d(lib):
    out = C.run_case(C.FlowSystem(lib, C.cart_grid([14, 14, 14]), sigma=2.0), lib)
    assert out["levels"] >= 3
    _report("cart 14^3 sigma 2", out)


@pytest.mark.parametrize("dim", [2, 3])
def test_block_systems(lib, dim):
    import porepy_amd as pa

    if dim == 2:
        g = pa.StructuredTriangleGrid([14, 14], [1.0, 1.0])
        g.compute_geometry()
    else:
        g = C.tet_grid(5)

    def expect(H):
        assert H[0]["block_size"] == dim and not H[0]["restrict_lanes"] and len(H) >= 2
    out = C.run_case(C.MechSystem(lib, g), lib, expect=expect)
    assert out["filter"][3] > 0, "the block filter dropped nothing"
    _report(f"mpsa bs={dim}", out)


def test_user_csr_unsorted_singleton_and_hub(lib):
    A, hub = C.edge_case_matrix()

    def expect(H):
        h = H[0]
        assert not h["sys"].has_sorted_indices
        sizes = np.bincount(h["agg"])
        assert sizes[h["agg"][-1]] == 1  # the diagonal-only row is an aggregate of its own
        # the hub's coarse row gathers more entries than the batched gather holds (kGalEpl per lane, 64 lanes):
        # the whole product takes the member-by-member path
        assert np.diff(h["A"].indptr)[hub] > h["gal_epl"] * 64
        assert h["galerkin_max_gather"] > h["gal_epl"] * 64
    _report("user csr edge cases", C.run_case(C.UserSystem(lib, A), lib, expect=expect))


def test_user_csr_without_locality(lib):
    A = C.no_locality_matrix()

    def expect(H):
        # (device: both window builds -- of the system and of the filtered operator, tried from 200 000 entries --
        # overflow and the products fall back to plain CSR)
        assert H[0]["sys"].nnz >= 200000 and H[0]["op"].nnz >= 200000 and not H[0]["window"]
        assert C.window_columns(H[0]["op"]) > 4096 and len(H) == 2
    out = C.run_case(C.UserSystem(lib, A), lib, env={"PFV_AMG_COARSE_TARGET": "1024"}, expect=expect)
    _report("user csr without locality", out)


def test_jacobi_fallback_on_a_stalled_coarsest_level(lib):
    def expect(H):
        assert len(H) == 2 and H[1]["n"] > H[0]["dense_max"] and not H[1]["dense_ok"] and "jacobi" in H[1]["path"]
    _report("stalled coarsening", C.run_case(C.UserSystem(lib, C.stalled_matrix()), lib, expect=expect))


def test_leading_block(lib):
    C.leading_block(lib)


def test_switch_matrix_scalar(lib):
    res = C.switch_matrix(lambda: C.FlowSystem(lib, C.tet_grid(10), seed=4), lib)
    assert res["default"]["levels"] >= 3
    for name, out in res.items():
        _report("switches tets 10^3 / " + name, out)


def test_switch_matrix_block(lib):
    res = C.switch_matrix(lambda: C.MechSystem(lib, C.tet_grid(6)), lib)
    assert res["default"]["levels"] >= 3
    for name, out in res.items():
        _report("switches mpsa 6^3 / " + name, out)


def test_state_sequence(lib):
    for tag, out in C.state_sequence(lib, 8):
        _report("state / " + tag, out)


def test_matching_switch_change_rematches(lib):
    assert C.matching_switch_change_rematches(lib, 8) >= 3


def test_different_pattern_with_equal_sizes_rebuilds_the_maps(lib):
    C.different_pattern_same_sizes(lib)


def test_mutations_of_the_reference_are_detected(lib):
    assert C.mutations(lib, 8)
