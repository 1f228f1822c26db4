"""Cases of the finest level's post-smoothing through AP = A_s P (PFV_AMG_POST_AP; csrc/amg.inc: amg_build_ap,
amg_post_ap), shared by the emulation suite (test_amg_ap_emulation.py) and the GPU suite (test_gpu_amg_ap.py).

The new launch replaces the prolongation and the smoothing product of level 0 where that level takes the two-launch
restriction (its t = A_s x0 is then in memory).  Small systems take the fused restriction on level 0 instead, so every
case here runs under PFV_AMG_FUSE_ROWS=0, which puts level 0 of a small system on the path the large systems take by
default; ``stats()["amg_ap_nnz"]`` tells that AP was built (and is compared with the count made on the host).

Every variant is judged by tests/_amg_cases.py (check_setup, check_cycle: bound = FACTOR x the float64-vs-longdouble
difference of the case); switch on against switch off must agree within the larger of the two bounds."""
import os

import numpy as np
import scipy.sparse as sps

import porepy_amd as pa
from tests import _amg_cases as C

LD = np.longdouble
BASE = {"PFV_AMG_FUSE_ROWS": "0", "PFV_AMG_REUSE": "0"}
SWITCH = "PFV_AMG_POST_AP"


def ap_entries(H0):
    """Entries of A_s P counted on the host: distinct aggregates among the columns of every row of the operator."""
    op, agg = H0["op"], H0["agg"]
    n = op.shape[0]
    S = sps.csr_matrix((np.ones(op.nnz), op.indices, op.indptr), shape=op.shape)
    Pm = sps.csr_matrix((np.ones(n), (np.arange(n), agg)), shape=(n, int(agg.max()) + 1))
    return int((S @ Pm).nnz)


def setup_and_apply(sysm, lib, env, V=None):
    with C.environment(env):
        sysm.ctx.amg_setup(0)
        H = C.read_hierarchy(sysm.ctx)
        setup = C.check_setup(H)
        V = C.case_vectors(H, 3) if V is None else V
        cyc = C.check_cycle(sysm.ctx, lib, H, V=V)
        ap = int(sysm.ctx.stats()["amg_ap_nnz"])
    return {"H": H, "setup": setup, "cycle": cyc, "ap_nnz": ap, "V": V}


def on_against_off(make_system, lib, env=None, expect_ap=True, expect=None):
    """Same system, switch off then on: each passes the pinned checks against its own read-out, the applied vectors
    agree within the larger bound, the hierarchies are equal."""
    sysm = make_system()
    off = setup_and_apply(sysm, lib, dict(BASE, **(env or {}), **{SWITCH: "0"}))
    on = setup_and_apply(sysm, lib, dict(BASE, **(env or {}), **{SWITCH: "1"}), V=off["V"])
    if expect is not None:
        expect(on["H"])
    assert "restrict_residual" not in on["H"][0]["path"]
    assert off["ap_nnz"] == 0
    if expect_ap:
        assert on["H"][0]["block_size"] == 1 and on["H"][0]["fp32"]
        assert on["ap_nnz"] == ap_entries(on["H"][0]), (on["ap_nnz"], ap_entries(on["H"][0]))
    else:
        assert on["ap_nnz"] == 0
    tol = max(on["cycle"]["bound"], off["cycle"]["bound"])
    diff = C.max_rel(on["cycle"]["Z"], off["cycle"]["Z"].astype(LD))
    print(f"post_ap on/off: rows {[h['n'] for h in on['H']]} ap_nnz {on['ap_nnz']} "
          f"({on['ap_nnz'] / on['H'][0]['n']:.2f} per row, operator {on['H'][0]['op'].nnz / on['H'][0]['n']:.2f}) "
          f"error on {on['cycle']['error']:.2e} off {off['cycle']['error']:.2e} bound {tol:.2e} on-off {diff:.2e}")
    assert diff <= tol, ("on against off", diff, tol)
    C.hierarchies_equal(off["H"], on["H"], tol)
    return on, off


def tets_w_cycle(lib, n=8):
    def expect(H):
        assert len(H) >= 3 and H[0]["gamma"] == 2 and "second_visit" in H[0]["path"]
    return on_against_off(lambda: C.FlowSystem(lib, C.tet_grid(n), seed=4), lib, {"PFV_AMG_GAMMA": "2"}, expect=expect)


def tets_v_cycle(lib, n=8):
    def expect(H):
        assert len(H) >= 3 and H[0]["gamma"] == 1 and "second_visit" not in H[0]["path"]
    return on_against_off(lambda: C.FlowSystem(lib, C.tet_grid(n), seed=4), lib, {"PFV_AMG_GAMMA": "1"}, expect=expect)


def cartesian_2d(lib):
    def expect(H):
        assert H[0]["n"] == 33 * 31 and H[0]["n"] % 64 != 0 and len(H) >= 2
    return on_against_off(lambda: C.FlowSystem(lib, C.cart_grid([33, 31])), lib, expect=expect)


def without_locality(lib):
    def expect(H):
        assert H[0]["op"].nnz >= 200000 and not H[0]["window"] and len(H) == 2
    return on_against_off(lambda: C.UserSystem(lib, C.no_locality_matrix()), lib, {"PFV_AMG_COARSE_TARGET": "1024"},
                          expect=expect)


def stalled(lib):
    def expect(H):
        assert len(H) == 2 and not H[1]["dense_ok"] and "jacobi" in H[1]["path"]
    return on_against_off(lambda: C.UserSystem(lib, C.stalled_matrix()), lib, expect=expect)


def long_rows(lib):
    """A hub row with several hundred entries after the filter: longer than the rows the build kernel ranks in LDS."""
    A, hub = C.edge_case_matrix()

    def expect(H):
        assert np.diff(H[0]["op"].indptr)[hub] > 128
    return on_against_off(lambda: C.UserSystem(lib, A), lib, expect=expect)


def block_system(lib):
    def expect(H):
        assert H[0]["block_size"] == 3
    return on_against_off(lambda: C.MechSystem(lib, C.tet_grid(5)), lib, expect_ap=False, expect=expect)


def fp64_fallback(lib, n=8):
    def expect(H):
        assert not any(h["fp32"] for h in H)
    return on_against_off(lambda: C.FlowSystem(lib, C.tet_grid(n), seed=4), lib, {"PFV_AMG_FP32": "0"}, expect_ap=False,
                          expect=expect)


def determinism(lib, n=8):
    """Two setups from the same values and two applies: the same bits."""
    S = C.FlowSystem(lib, C.tet_grid(n), seed=4)
    env = dict(BASE, **{SWITCH: "1", "PFV_AMG_GAMMA": "2"})
    with C.environment(env):
        S.ctx.amg_setup(0)
        H = C.read_hierarchy(S.ctx)
        assert int(S.ctx.stats()["amg_ap_nnz"]) > 0
        V = C.case_vectors(H, 3)
        Z1 = C.apply_cycle(S.ctx, lib, V)
        Z2 = C.apply_cycle(S.ctx, lib, V)
        S.ctx.amg_setup(0)
        assert int(S.ctx.stats()["amg_ap_nnz"]) > 0
        Z3 = C.apply_cycle(S.ctx, lib, V)
    assert np.array_equal(Z1, Z2), "two applies differ"
    assert np.array_equal(Z1, Z3), "two setups from the same values differ"
    return True


def solve_on_against_off(lib, g, rtol=1e-12):
    """BiCGStab + AMG on the heterogeneous anisotropic tensor of _parity.amg_fused_cycle_is_the_same_operator, switch on
    against off, by that test's criteria: iterations within 1, solutions to 1e-9 relative."""
    rng = np.random.default_rng(4)
    sc = np.exp(0.5 * rng.standard_normal(g.num_cells))
    kw = dict(kxx=sc, kyy=3 * sc, kxy=0.3 * sc)
    if g.dim == 3:
        kw.update(kzz=0.4 * sc, kyz=0.1 * sc)
    bf = g.get_all_boundary_faces()
    xf = g.face_centers[0, bf]
    dirf = bf[(xf < 1e-9) | (xf > g.nodes[0].max() - 1e-9)]
    bv = np.zeros(g.num_faces)
    bv[dirf] = g.face_centers[0, dirf]
    res = {}
    for sw in ("0", "1"):
        with C.environment(dict(BASE, **{SWITCH: sw, "PFV_AMG_GAMMA": "2"})):
            data = pa.initialize_data({}, "flow", {"second_order_tensor": pa.SecondOrderTensor(**kw),
                                                   "bc": pa.BoundaryCondition(g, dirf, ["dir"] * dirf.size),
                                                   "bc_values": bv})
            d = pa.Mpfa("flow", library=lib)
            d.discretize(g, data)
            d.assemble_matrix_rhs(g, data)
            x, info = d.solve(g, data, source=g.cell_volumes, method="bicgstab", rtol=rtol, precond="amg")
            assert info["converged"], (sw, info)
            st = d.context(g).stats()
            res[sw] = (x, int(info["iterations"]), int(st["amg_ap_nnz"]), int(st["amg_levels"]),
                       int(st.get("solve_launches", 0)))
            d.context(g).close()
    (x0, it0, ap0, lev, l0), (x1, it1, ap1, _, l1) = res["0"], res["1"]
    print(f"post_ap solve: iterations off {it0} on {it1}, launches off {l0} on {l1}, ap_nnz {ap1}")
    assert lev >= 3 and ap0 == 0 and ap1 > 0
    assert abs(it1 - it0) <= 1, (it0, it1)
    assert np.linalg.norm(x1 - x0) <= 1e-9 * np.linalg.norm(x0)
    if l0 > 0:  # (the device build counts launches: one fewer per cycle)
        assert l1 < l0, (l0, l1)
    return it0, it1
