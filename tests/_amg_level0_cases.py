"""Cases of level 0 of the AMG cycle on its AP path (csrc/amg.inc: amg_cycle, amg_residual_l0, amg_restrict,
amg_post_ap; csrc/linalg.inc: krylov_solve), shared by the emulation suite (test_amg_level0_emulation.py) and the GPU
suite (test_gpu_amg_level0.py).  Three switches, default on, each restoring the earlier launches at 0:

  PFV_AMG_L0_RESIDUAL       the level's product leaves d = b - A_s x0; restriction and post-smoothing read d alone
  PFV_AMG_L0_LANES4         ... formed by 4 lanes per row where level 0 has windows and short rows (device only)
  PFV_AMG_KRYLOV_PRESMOOTH  BiCGStab's two updates write the cycle's first smoothing step

Every case runs under PFV_AMG_FUSE_ROWS=0 and PFV_AMG_REUSE=0 (level 0 of a small system on the path the large systems
take) and is judged by tests/_amg_cases.py as it stands: check_setup, check_cycle (bound = 16 x the float64-vs-longdouble
difference of the case, at most 1e-10); all switches on against all off must agree within the larger of the two bounds,
and the hierarchies must be equal."""
import numpy as np

import porepy_amd as pa
from tests import _amg_ap_cases as AP
from tests import _amg_cases as C

LD = np.longdouble
BASE = dict(AP.BASE)
SWITCHES = ("PFV_AMG_L0_RESIDUAL", "PFV_AMG_L0_LANES4", "PFV_AMG_KRYLOV_PRESMOOTH")
ALL_ON = {k: "1" for k in SWITCHES}
ALL_OFF = {k: "0" for k in SWITCHES}


def setup_and_apply(sysm, lib, env, V=None):
    with C.environment(env):
        sysm.ctx.amg_setup(0)
        H = C.read_hierarchy(sysm.ctx)
        setup = C.check_setup(H)
        V = C.case_vectors(H, 3) if V is None else V
        cyc = C.check_cycle(sysm.ctx, lib, H, V=V)
        ap = int(sysm.ctx.stats()["amg_ap_nnz"])
    return {"H": H, "setup": setup, "cycle": cyc, "ap_nnz": ap, "V": V}


def on_against_off(make_system, lib, env=None, expect=None, expect_ap=True):
    """Same system, all switches off then on."""
    sysm = make_system()
    off = setup_and_apply(sysm, lib, dict(BASE, **(env or {}), **ALL_OFF))
    on = setup_and_apply(sysm, lib, dict(BASE, **ALL_ON, **(env or {})), V=off["V"])
    if expect is not None:
        expect(on["H"])
    assert "restrict_residual" not in on["H"][0]["path"]
    if expect_ap:
        assert on["H"][0]["block_size"] == 1 and on["H"][0]["fp32"]
        assert on["ap_nnz"] == off["ap_nnz"] == AP.ap_entries(on["H"][0])
    else:
        assert on["ap_nnz"] == 0 and off["ap_nnz"] == 0
    tol = max(on["cycle"]["bound"], off["cycle"]["bound"])
    diff = C.max_rel(on["cycle"]["Z"], off["cycle"]["Z"].astype(LD))
    print(f"level 0 on/off: rows {[h['n'] for h in on['H']]} window {bool(on['H'][0]['window'])} "
          f"ap_nnz {on['ap_nnz']} error on {on['cycle']['error']:.2e} off {off['cycle']['error']:.2e} "
          f"bound {tol:.2e} on-off {diff:.2e}")
    assert diff <= tol, ("on against off", diff, tol)
    C.hierarchies_equal(off["H"], on["H"], tol)
    return on, off


def tets_w_cycle(lib, n=8):
    def expect(H):
        assert H[0]["n"] == 6 * n ** 3 and H[0]["n"] % 256 == 0
        assert len(H) >= 3 and H[0]["gamma"] == 2 and "second_visit" in H[0]["path"]
    return on_against_off(lambda: C.FlowSystem(lib, C.tet_grid(n), seed=4), lib, {"PFV_AMG_GAMMA": "2"}, expect=expect)


def tets_v_cycle(lib, n=8):
    def expect(H):
        assert len(H) >= 3 and H[0]["gamma"] == 1 and "second_visit" not in H[0]["path"]
    return on_against_off(lambda: C.FlowSystem(lib, C.tet_grid(n), seed=4), lib, {"PFV_AMG_GAMMA": "1"}, expect=expect)


def cartesian_last_window_short(lib):
    def expect(H):
        assert H[0]["n"] == 1023 and len(H) >= 2
    return on_against_off(lambda: C.FlowSystem(lib, C.cart_grid([33, 31])), lib, expect=expect)


def cartesian_last_group_of_three(lib):
    def expect(H):
        assert H[0]["n"] == 957 and (957 + 63) // 64 == 15 and len(H) >= 2
    return on_against_off(lambda: C.FlowSystem(lib, C.cart_grid([33, 29])), lib, expect=expect)


def long_rows(lib):
    A, hub = C.edge_case_matrix()

    def expect(H):
        assert np.diff(H[0]["op"].indptr)[hub] > 128
    return on_against_off(lambda: C.UserSystem(lib, A), lib, expect=expect)


def windowed_many_blocks(lib):
    """tet_grid(16): 24 576 rows, 384 row blocks with windows: the residual form of the windowed product (device)."""
    def expect(H):
        assert H[0]["n"] == 24576 and H[0]["window"] and len(H) >= 3
    return on_against_off(lambda: C.FlowSystem(lib, C.tet_grid(16, 0.015), seed=4), lib, {"PFV_AMG_GAMMA": "2"},
                          expect=expect)


def without_locality(lib):
    def expect(H):
        assert H[0]["op"].nnz >= 200000 and not H[0]["window"] and len(H) == 2
    return on_against_off(lambda: C.UserSystem(lib, C.no_locality_matrix()), lib, {"PFV_AMG_COARSE_TARGET": "1024"},
                          expect=expect)


def stalled(lib):
    def expect(H):
        assert len(H) == 2 and not H[1]["dense_ok"] and "jacobi" in H[1]["path"]
    return on_against_off(lambda: C.UserSystem(lib, C.stalled_matrix()), lib, expect=expect)


def _same_launches(sysm, lib, env, n=None):
    """A system that takes none of it: solves with all switches on and all off are the same launches and bits."""
    res = {}
    for tag, sw in (("off", ALL_OFF), ("on", ALL_ON)):
        with C.environment(dict(BASE, **env, **sw)):
            x, info = sysm.ctx.solve(method="bicgstab", rtol=1e-8, maxit=400, precond="amg", n=n, raise_on_fail=False)
            st = sysm.ctx.stats()
            res[tag] = (np.array(x), int(info["iterations"]), int(st.get("solve_launches", 0)))
    (x0, it0, l0), (x1, it1, l1) = res["off"], res["on"]
    print(f"path unchanged: iterations {it0} / {it1}, launches {l0} / {l1}")
    assert it0 > 0 and it0 == it1 and l0 == l1
    assert np.array_equal(x0, x1)


def block_system(lib):
    def expect(H):
        assert H[0]["block_size"] == 3
    g = C.tet_grid(5)
    on_against_off(lambda: C.MechSystem(lib, g), lib, expect_ap=False, expect=expect)
    S = C.MechSystem(lib, g)
    # (the case's boundary values are zero: a right-hand side to iterate on)
    S.data[pa.PARAMETERS]["mechanics"]["bc_values"] = np.random.default_rng(3).standard_normal(g.dim * g.num_faces)
    S.d.assemble_matrix_rhs(g, S.data)
    _same_launches(S, lib, {}, n=S.n)


def fp64_fallback(lib, n=8):
    def expect(H):
        assert not any(h["fp32"] for h in H)
    make = lambda: C.FlowSystem(lib, C.tet_grid(n), seed=4)
    on_against_off(make, lib, {"PFV_AMG_FP32": "0"}, expect_ap=False, expect=expect)
    _same_launches(make(), lib, {"PFV_AMG_FP32": "0"})


def determinism(lib, n=8):
    """Two setups from the same values and two applies: the same bits."""
    S = C.FlowSystem(lib, C.tet_grid(n), seed=4)
    with C.environment(dict(BASE, **ALL_ON, **{"PFV_AMG_GAMMA": "2"})):
        S.ctx.amg_setup(0)
        H = C.read_hierarchy(S.ctx)
        V = C.case_vectors(H, 3)
        Z1 = C.apply_cycle(S.ctx, lib, V)
        Z2 = C.apply_cycle(S.ctx, lib, V)
        S.ctx.amg_setup(0)
        Z3 = C.apply_cycle(S.ctx, lib, V)
    assert np.array_equal(Z1, Z2), "two applies differ"
    assert np.array_equal(Z1, Z3), "two setups from the same values differ"
    return True


def residual_form_keeps_the_coarse_rhs(lib, make_system=None, env=None):
    """PFV_AMG_L0_RESIDUAL alone (the product stays on its 8 lanes): the restriction adds the same numbers in the same
    order, so the right-hand side of level 1 has the bits of the two-gather form."""
    S = (make_system or (lambda: C.FlowSystem(lib, C.tet_grid(8), seed=4)))()
    bc = {}
    for sw in ("0", "1"):
        e = dict(BASE, **ALL_OFF, **(env or {}), **{"PFV_AMG_GAMMA": "2"})
        e["PFV_AMG_L0_RESIDUAL"] = sw
        with C.environment(e):
            S.ctx.amg_setup(0)
            H = C.read_hierarchy(S.ctx)
            assert int(S.ctx.stats()["amg_ap_nnz"]) > 0 and len(H) >= 2
            V = C.case_vectors(H, 3)
            rows = []
            for v in V[:5]:
                z = C.apply_cycle(S.ctx, lib, v)
                assert np.all(np.isfinite(z))
                rows.append(S.ctx.amg_level_rhs(1))
            bc[sw] = np.array(rows)
    assert np.abs(bc["0"]).max() > 0
    assert np.array_equal(bc["0"], bc["1"]), "coarse right-hand side differs"
    return True


def _flow_problem(g):
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
    return {"second_order_tensor": pa.SecondOrderTensor(**kw), "bc": pa.BoundaryCondition(g, dirf, ["dir"] * dirf.size),
            "bc_values": bv}


def _solve(lib, g, env, rtol):
    """BiCGStab + AMG on the heterogeneous anisotropic tensor of _amg_ap_cases.solve_on_against_off"""
    with C.environment(dict(BASE, **{"PFV_AMG_GAMMA": "2"}, **env)):
        data = pa.initialize_data({}, "flow", _flow_problem(g))
        d = pa.Mpfa("flow", library=lib)
        d.discretize(g, data)
        d.assemble_matrix_rhs(g, data)
        x, info = d.solve(g, data, source=g.cell_volumes, method="bicgstab", rtol=rtol, precond="amg")
        assert info["converged"], (env, info)
        st = d.context(g).stats()
        out = {"x": np.array(x), "it": int(info["iterations"]), "ap": int(st["amg_ap_nnz"]),
               "levels": int(st["amg_levels"]), "launches": int(st.get("solve_launches", 0))}
        d.context(g).close()
    return out


def presmoothing_in_the_krylov_updates(lib, g, rtol=1e-12):
    """PFV_AMG_KRYLOV_PRESMOOTH on against off (the other switches on): the same expression on the same numbers, so
    equal iteration counts and solutions bit for bit, and two launches fewer per iteration."""
    off = _solve(lib, g, dict(ALL_ON, PFV_AMG_KRYLOV_PRESMOOTH="0"), rtol)
    on = _solve(lib, g, ALL_ON, rtol)
    print(f"krylov presmooth: iterations off {off['it']} on {on['it']}, launches off {off['launches']} on {on['launches']}")
    assert on["levels"] >= 3 and on["ap"] > 0 and off["ap"] == on["ap"]
    assert on["it"] == off["it"], (off["it"], on["it"])
    assert np.array_equal(on["x"], off["x"])
    if lib.pfv_is_device_build():  # (the device build counts launches)
        assert off["launches"] > 0
        assert off["launches"] - on["launches"] == 2 * on["it"], (off["launches"], on["launches"], on["it"])
    return True


def solve_all_on_against_all_off(lib, g, rtol=1e-12):
    """By the criteria of _amg_ap_cases.solve_on_against_off: iterations within 1, solutions to 1e-9 relative."""
    off = _solve(lib, g, ALL_OFF, rtol)
    on = _solve(lib, g, ALL_ON, rtol)
    print(f"level 0 solve: iterations off {off['it']} on {on['it']}, launches off {off['launches']} on {on['launches']}")
    assert on["levels"] >= 3 and on["ap"] > 0 and off["ap"] == on["ap"]
    assert abs(on["it"] - off["it"]) <= 1, (off["it"], on["it"])
    assert np.linalg.norm(on["x"] - off["x"]) <= 1e-9 * np.linalg.norm(off["x"])
    if off["launches"] > 0:
        assert on["launches"] < off["launches"]
    return True
