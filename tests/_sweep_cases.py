"""Cases of the flow-ordered sweep (PFV_PRECOND_SWEEP, csrc/sweep.inc), shared by the emulation suite
(test_sweep_emulation.py) and the GPU suite (test_gpu_sweep.py): each takes the library to run on.

Judges: for the order, ``flow_order`` below -- a numpy restatement of the two peels on the edge list; for solutions,
scipy's spsolve on the matrix the library exports."""
import contextlib
import os

import numpy as np
import scipy.sparse as sps
import scipy.sparse.linalg as spla

import porepy_amd as pa
from porepy_amd import _lib
from tests import _advdiff_cases as AD
from tests import _upwind_cases as UP
from tests._upwind_cases import KW, data_for, geo, line_grid, tets

VEL = [0.6, -0.3, 0.45]


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


# ---- the judge of the order ---------------------------------------------------------------------------------------
def edges(g, q):
    """(up, dn) of every interior face with q != 0 and q not NaN; upstream = the cell with sign +1 where q > 0."""
    cf = sps.csc_matrix(g.cell_faces)
    nf = cf.shape[0]
    fi, ci, sg = sps.find(cf)
    side = -np.ones((2, nf), dtype=np.int64)
    side[0, fi[sg > 0]] = ci[sg > 0]
    side[1, fi[sg < 0]] = ci[sg < 0]
    q = np.asarray(q, dtype=float)
    with np.errstate(invalid="ignore"):
        ok = (side[0] >= 0) & (side[1] >= 0) & ~np.isnan(q) & (q != 0)
        pos = q > 0
    return np.where(pos, side[0], side[1])[ok], np.where(pos, side[1], side[0])[ok]


def _peel(n, src, dst, alive):
    """Passes of: remove the alive cells without an edge coming in from an alive cell.  Returns the pass of every cell
    (-1: never removed) and the number of passes."""
    keep = alive[src] & alive[dst]
    src, dst = src[keep], dst[keep]
    deg = np.bincount(dst, minlength=n)
    out = -np.ones(n, dtype=np.int64)
    front = np.flatnonzero(alive & (deg == 0))
    p = 0
    while front.size:
        out[front] = p
        hit = dst[np.isin(src, front)]
        np.subtract.at(deg, hit, 1)
        cand = np.unique(hit)
        front = cand[deg[cand] == 0]
        p += 1
    return out, p


def flow_order(nc, up, dn):
    fwd, nfwd = _peel(nc, up, dn, np.ones(nc, dtype=bool))
    rest = fwd < 0
    bwd, nbwd = _peel(nc, dn, up, rest)  # (the same peel on the reversed edges of what is left)
    core = rest & (bwd < 0)
    has_core = int(core.any())
    level = np.where(~rest, fwd, np.where(core, nfwd, nfwd + has_core + (nbwd - 1 - bwd)))
    return {"level": level, "order": np.argsort(level, kind="stable"), "levels": nfwd + has_core + nbwd,
            "core_cells": int(core.sum()), "core_level": nfwd if has_core else -1, "nfwd": nfwd, "nbwd": nbwd,
            "core": core}


def same_order(info, ref):
    assert info["levels"] == ref["levels"], (info["levels"], ref["levels"])
    assert info["core_cells"] == ref["core_cells"] and info["core_level"] == ref["core_level"]
    assert np.array_equal(info["level"], ref["level"])
    assert np.array_equal(info["order"], ref["order"])
    assert np.array_equal(info["order"], np.argsort(info["level"], kind="stable"))


# ---- fluxes ------------------------------------------------------------------------------------------------------
def cyclic_field(n=12):
    """CartGrid([n, n], [1, 1]): a drift plus a vortex of radius 0.3 around the centre -- a cyclic core inside an
    acyclic through-flow."""
    g = geo(pa.CartGrid([n, n], [1.0, 1.0]))
    x, y = g.face_centers[0] - 0.5, g.face_centers[1] - 0.5
    inside = np.hypot(x, y) < 0.3
    v = np.vstack([1.0 + 6.0 * inside * (-y), 0.2 + 6.0 * inside * x])
    return g, np.sum(v * g.face_normals[:2], axis=0)


def rotation(n=8):
    g = geo(pa.CartGrid([n, n]))
    c = 0.5 * n
    x, y = g.face_centers[0] - c, g.face_centers[1] - c
    return g, np.sum(np.vstack([-y, x]) * g.face_normals[:2], axis=0)


def order_case(name):
    """(grid, flux, environment, expected levels / core of the issue's table or None)"""
    up = pa.Upwind(KW)
    if name in ("tets3", "tets4", "tets6", "tets6_in_place"):
        g = tets(int(name[4]))
        return g, up.darcy_flux(g, VEL), ({"PFV_REORDER": 0} if name.endswith("in_place") else {}), \
            {3: (18, 0), 4: (27, 0), 6: (43, 0)}[int(name[4])]
    if name == "potential6":
        g = tets(6)
        p = np.random.default_rng(2).random(g.num_cells)
        return g, -(sps.csr_matrix(g.cell_faces) @ p), {}, None
    if name == "cyclic12":
        g, q = cyclic_field()
        return g, q, {}, (None, 45)
    if name == "rotation8":
        g, q = rotation()
        return g, q, {}, (1, 64)
    if name == "line":
        g = line_grid(16, 2.0)
        return g, np.ones(g.num_faces), {}, (16, 0)
    raise KeyError(name)


ORDER_CASES = ["tets3", "tets6", "tets6_in_place", "potential6", "cyclic12", "rotation8", "line"]


def _solved(lib, g, q, rtol=1e-12, method="gmres", precond="sweep", seed=1, bv=None):
    """One solve of (diag(acc) + A) c = acc c_old - b_ref with every boundary face Dirichlet; returns what the judge
    needs next to it."""
    rng = np.random.default_rng(seed)
    if bv is None:
        bv = np.zeros(g.num_faces)
        bf = g.get_all_boundary_faces()
        bv[bf] = rng.random(bf.size)
    acc = np.asarray(g.cell_volumes, dtype=float) * (0.5 + rng.random(g.num_cells)) / 0.05
    c_old = rng.random(g.num_cells)
    data = data_for(q, None, bv)
    up = pa.Upwind(KW, library=lib)
    up.discretize(g, data)
    A, bref = up.assemble_matrix_rhs(g, data)
    c, info = up.solve(g, data, accumulation=acc, c_old=c_old, method=method, rtol=rtol, precond=precond)
    ref = spla.spsolve((sps.diags(acc) + sps.csr_matrix(A)).tocsc(), acc * c_old - bref)
    return up, c, info, ref


# ---- 1. order parity -----------------------------------------------------------------------------------------------
def order_parity(lib, name):
    g, q, environment, expect = order_case(name)
    ref = flow_order(g.num_cells, *edges(g, q))
    if expect is not None:  # the graph facts the case stands for, on the judge
        assert expect[0] is None or ref["levels"] == expect[0], ref["levels"]
        assert ref["core_cells"] == expect[1], ref["core_cells"]
    else:
        assert ref["core_cells"] == 0 and 7 <= ref["levels"] <= 13, ref["levels"]
    with env(**environment):
        up, c, info, sol = _solved(lib, g, q)
        ctx = up.context(g)
        st = ctx.stats()
        got = ctx.sweep_info()
    print(f"{name}: {g.num_cells} cells, {got['levels']} levels, core {got['core_cells']} at {got['core_level']}, "
          f"renumbered {st['solve_renumbered']}, {st['sweep_launches']} launches per sweep")
    if name == "tets6":
        assert st["solve_renumbered"] == 1  # above PFV_REORDER_MIN_CELLS: the permuted branch
    if name in ("tets3", "tets6_in_place", "cyclic12", "rotation8", "line"):
        assert st["solve_renumbered"] == 0
    same_order(got, ref)
    assert st["sweep_levels"] == ref["levels"] and st["sweep_core_cells"] == ref["core_cells"]
    assert info["converged"] and np.abs(c - sol).max() <= 1e-10 * np.abs(sol).max()
    if name == "cyclic12":
        # forward peel alone leaves 89 cells; the core sits between 14 forward and 12 backward levels
        assert (ref["nfwd"], ref["nbwd"], ref["core_level"]) == (14, 12, 14)
        assert int((ref["level"] >= ref["nfwd"]).sum()) == 89
        non_core = ~ref["core"]
        assert np.array_equal(got["level"][non_core], ref["level"][non_core])
        assert np.all(got["level"][ref["core"]] == 14)


def stagnant_faces_make_no_edge(lib):
    """q = 0, -0.0 and NaN on interior faces of the tets(3) flux: none of them is an edge."""
    g = tets(3)
    q0 = pa.Upwind(KW).darcy_flux(g, VEL)
    interior = np.setdiff1d(np.arange(g.num_faces), g.get_all_boundary_faces())
    pick = interior[np.random.default_rng(4).permutation(interior.size)[:30]]
    q = q0.copy()
    q[pick[:15]] = 0.0
    q[pick[15:]] = -0.0
    ref = flow_order(g.num_cells, *edges(g, q))
    base = flow_order(g.num_cells, *edges(g, q0))
    assert ref["core_cells"] == 0 and not np.array_equal(ref["level"], base["level"])
    up, c, info, sol = _solved(lib, g, q)
    same_order(up.context(g).sweep_info(), ref)
    assert info["converged"] and info["iterations"] == 1
    assert np.abs(c - sol).max() <= 1e-12 * np.abs(sol).max()
    # NaN: the upstream cell's diagonal is NaN, so the solve is refused as ever -- after the order was built
    qn = q.copy()
    qn[pick[:5]] = np.nan
    refn = flow_order(g.num_cells, *edges(g, qn))
    assert edges(g, qn)[0].size == edges(g, q0)[0].size - 30
    data = data_for(qn, None, np.zeros(g.num_faces))
    upn = pa.Upwind(KW, library=lib)
    upn.discretize(g, data)
    try:
        upn.solve(g, data, accumulation=np.ones(g.num_cells), c_old=np.ones(g.num_cells), precond="sweep")
    except pa.PorefvError as e:
        assert e.status == 5 and "zero diagonal" in e.message
    else:
        raise AssertionError("a NaN diagonal must be refused")
    same_order(upn.context(g).sweep_info(), refn)


# ---- 2. the direct step is exact -------------------------------------------------------------------------------------
def _injection(g):
    q = pa.Upwind(KW).darcy_flux(g, VEL)
    bf = g.get_all_boundary_faces()
    inflow_value = np.zeros(g.num_faces)
    inflow_value[bf] = 1.0  # (used on the Dirichlet inflow faces only)
    acc = 0.25 * np.asarray(g.cell_volumes, dtype=float) / 0.02
    src = np.zeros(g.num_cells)
    src[g.num_cells // 2] = 1.0
    return q, pa.BoundaryCondition(g, bf, ["dir"] * bf.size), inflow_value, acc, src


def _three_steps(lib, g, bv, source, precond="sweep"):
    q, bc, _, acc, _ = _injection(g)
    data = data_for(q, bc, bv)
    up = pa.Upwind(KW, library=lib)
    up.discretize(g, data)
    A, bref = up.assemble_matrix_rhs(g, data)
    c, info = up.advance(g, data, np.zeros(g.num_cells), 3, acc, source=source, rtol=1e-13, precond=precond)
    st = up.context(g).stats()
    M = (sps.diags(acc) + sps.csr_matrix(A)).tocsc()
    ref = np.zeros(g.num_cells)
    for _ in range(3):
        ref = spla.spsolve(M, acc * ref - bref + (0.0 if source is None else source))
    return up, data, c, info, st, ref, (M, acc, bref)


def direct_step_exact(lib, n=4):
    g = tets(n)
    q, _, inflow, acc, src = _injection(g)
    assert flow_order(g.num_cells, *edges(g, q))["core_cells"] == 0
    for what, bv, source in (("Dirichlet inflow 1", inflow, None), ("one source cell, from rest", np.zeros(g.num_faces), src)):
        up, data, c, info, st, ref, (M, _, bref) = _three_steps(lib, g, bv, source)
        err = np.abs(c - ref).max() / np.abs(ref).max()
        print(f"direct sweep, {what}: max-norm relative error {err:.2e} after 3 steps, "
              f"{st['sweep_levels']} levels, {st['sweep_launches']} launches per sweep")
        assert info["steps_done"] == 3 and info["converged"] and info["iterations"] == 1
        assert st["sweep_direct_steps"] == 3 and st["sweep_direct_fallbacks"] == 0
        assert st["transport_gmres_retries"] == 0 and st["transport_iterations"] == 3
        assert err <= 1e-12
        # the same step through solve()
        c_old = np.random.default_rng(8).random(g.num_cells)
        c1, i1 = up.solve(g, data, accumulation=acc, c_old=c_old, source=source, precond="sweep", rtol=1e-13)
        s1 = up.context(g).stats()
        r1 = spla.spsolve(M, acc * c_old - bref + (0.0 if source is None else source))
        assert i1["iterations"] == 1 and i1["converged"] and s1["sweep_direct_steps"] == 1
        assert i1["rel_residual"] <= 1e-13
        assert np.abs(c1 - r1).max() <= 1e-12 * np.abs(r1).max()


def euler_closed_form(lib):
    """The 1-D set-up of _upwind_cases.euler_closed_form, stepped with the sweep, against its recursion."""
    n, qv, dt, phi = 16, 0.7, 0.05, 0.3
    g = line_grid(n, 2.0)
    bc = pa.BoundaryCondition(g, g.get_all_boundary_faces(), ["dir", "dir"])
    bv = np.zeros(g.num_faces)
    bv[0] = 1.0
    acc = phi * g.cell_volumes / dt
    data = data_for(qv * np.ones(g.num_faces), bc, bv)
    up = pa.Upwind(KW, library=lib)
    up.discretize(g, data)
    nu = qv / acc
    c = np.zeros(n)
    for _ in range(10):
        new = np.empty(n)
        for i in range(n):
            new[i] = (c[i] + nu[i] * (new[i - 1] if i else 1.0)) / (1 + nu[i])
        c = new
    got, info = up.advance(g, data, np.zeros(n), 10, acc, rtol=1e-13, precond="sweep")
    st = up.context(g).stats()
    assert info["steps_done"] == 10 and st["sweep_direct_steps"] == 10 and st["transport_gmres_retries"] == 0
    assert st["sweep_levels"] == n
    assert np.abs(got - c).max() <= 1e-12


# ---- 3. a core still solves -------------------------------------------------------------------------------------------
def core_still_solves(lib):
    g, q = cyclic_field()
    ref = flow_order(g.num_cells, *edges(g, q))
    assert 0 < ref["core_cells"] < g.num_cells
    up, c, info, sol = _solved(lib, g, q, rtol=1e-12, method="gmres", precond="sweep")
    st = up.context(g).stats()
    _, cj, ij, _ = _solved(lib, g, q, rtol=1e-12, method="gmres", precond="jacobi")
    print(f"12 x 12 with a core of {st['sweep_core_cells']}: GMRES iterations sweep {info['iterations']}, "
          f"jacobi {ij['iterations']}")
    assert info["converged"] and ij["converged"]
    assert np.abs(c - sol).max() <= 1e-10 * np.abs(sol).max()
    assert st["sweep_core_cells"] == 45 and st["sweep_direct_steps"] == 0
    assert info["iterations"] < ij["iterations"]
    # all core
    g, q = rotation()
    assert flow_order(g.num_cells, *edges(g, q))["core_cells"] == g.num_cells
    up, c, info, sol = _solved(lib, g, q, rtol=1e-12, method="gmres", precond="sweep")
    st = up.context(g).stats()
    assert info["converged"] and st["sweep_core_cells"] == 64 and st["sweep_levels"] == 1
    assert np.abs(c - sol).max() <= 1e-10 * np.abs(sol).max()


# ---- 4. advection-diffusion -------------------------------------------------------------------------------------------
def advdiff(lib, scheme, n=4):
    g = tets(n)
    D = float(np.linalg.norm(VEL)) / n / 50.0  # cell Peclet number |v| h / D = 50
    pr = AD.problem(g, diffusivity=D, velocity=tuple(VEL))
    bf = g.get_all_boundary_faces()
    pr["bc"] = pr["par"]["bc"] = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)  # (so that -q has Dirichlet inflow too)
    pr["bv"] = pr["par"]["bc_values"] = np.where(pr["bc"].is_dir, 0.25 + np.random.default_rng(6).random(g.num_faces), 0.0)
    ad, data = AD.discretized(lib, g, pr, scheme)
    ctx = ad.context(g)
    A, b = AD.host_system(g, data[pa.DISCRETIZATION_MATRICES][KW], pr)
    ref1 = AD.host_steps(A, b, pr["acc"], pr["c0"], pr["src"], 1)
    ref3 = AD.host_steps(A, b, pr["acc"], pr["c0"], pr["src"], 3)
    order = flow_order(g.num_cells, *edges(g, pr["q"]))
    assert order["core_cells"] == 0
    its = {}
    for method in ("bicgstab", "gmres"):
        c, info = ad.solve(g, data, accumulation=pr["acc"], c_old=pr["c0"], source=pr["src"], method=method,
                           precond="sweep", rtol=1e-12)
        its[method] = info["iterations"]
        assert info["converged"] and np.abs(c - ref1).max() <= 1e-10
        assert ctx.stats()["sweep_direct_steps"] == 0  # (a preconditioner here, never the direct path)
        same_order(ctx.sweep_info(), order)
        c, info = ad.advance(g, data, pr["c0"], 3, pr["acc"], source=pr["src"], method=method, precond="sweep", rtol=1e-12)
        st = ctx.stats()
        assert info["steps_done"] == 3 and st["advdiff_precond_fallbacks"] == 0
        assert np.abs(c - ref3).max() <= 1e-10
    cj, ij = ad.solve(g, data, accumulation=pr["acc"], c_old=pr["c0"], source=pr["src"], method="gmres",
                      precond="jacobi", rtol=1e-12)
    print(f"advection-diffusion ({scheme}, Peclet 50): GMRES iterations sweep {its['gmres']}, jacobi {ij['iterations']}; "
          f"BiCGStab with sweep {its['bicgstab']}")
    assert np.abs(cj - ref1).max() <= 1e-10
    assert its["gmres"] < ij["iterations"]
    # the reversed flux on the same discretization: the reversed order
    data[pa.PARAMETERS][KW]["darcy_flux"] = -pr["q"]
    ad.update_flux(g, data, accumulation=pr["acc"], c_old=pr["c0"], source=pr["src"])
    c, info = ctx.solve(method="gmres", rtol=1e-12, precond="sweep")
    Ar, br = AD.host_system(g, data[pa.DISCRETIZATION_MATRICES][KW], pr, q=-pr["q"])
    refr = AD.host_steps(Ar, br, pr["acc"], pr["c0"], pr["src"], 1)
    rev = flow_order(g.num_cells, *edges(g, -pr["q"]))
    assert not np.array_equal(rev["level"], order["level"])
    same_order(ctx.sweep_info(), rev)
    assert info["converged"] and np.abs(c - refr).max() <= 1e-10


# ---- 5. determinism and the merged form --------------------------------------------------------------------------------
def deterministic_and_merged(lib, n=6):
    g = tets(n)
    _, _, _, _, src = _injection(g)
    runs = []
    for environment in ({}, {}, {"PFV_SWEEP_MERGE": 0}, {"PFV_SWEEP_MERGE_ROWS": 24}):
        with env(**environment):
            up, _, c, info, st, ref, _ = _three_steps(lib, g, np.zeros(g.num_faces), src)
            runs.append((c, up.context(g).sweep_info(), st["sweep_launches"], st["sweep_levels"]))
        assert info["steps_done"] == 3 and st["sweep_direct_steps"] == 3
        assert np.abs(c - ref).max() <= 1e-12 * np.abs(ref).max()
    print("launches per sweep (merged, merged, one per level, runs of levels <= 24 rows):", [r[2] for r in runs])
    for c, info, _, _ in runs[1:]:
        assert c.tobytes() == runs[0][0].tobytes()
        for k in ("level", "order"):
            assert np.array_equal(info[k], runs[0][1][k])
        assert {k: info[k] for k in ("levels", "core_cells", "core_level")} == \
            {k: runs[0][1][k] for k in ("levels", "core_cells", "core_level")}
    assert runs[2][2] == runs[2][3]  # one launch per level
    assert runs[0][2] < runs[3][2] < runs[2][2]


# ---- 6. errors and staleness -------------------------------------------------------------------------------------------
def errors(lib):
    import pytest

    g = tets(3)
    # a flow system and a user system: not what the sweep is for
    fdata, _ = UP.flow_problem(g, np.random.default_rng(3))
    mp = pa.Mpfa("flow", library=lib)
    mp.discretize(g, fdata)
    mp.assemble_matrix_rhs(g, fdata)
    ctx = mp.context(g)
    with pytest.raises(pa.PorefvError) as e:
        ctx.solve(precond="sweep")
    assert e.value.status == 5 and "PFV_PRECOND_SWEEP" in e.value.message
    with pytest.raises(pa.PorefvError) as e:
        ctx.sweep_info()
    assert e.value.status == 4
    user = _lib.Context(0, lib)
    user.set_system(sps.eye(5, format="csr") * 2.0, np.ones(5))
    with pytest.raises(pa.PorefvError) as e:
        user.solve(precond="sweep")
    assert e.value.status == 5
    x, info = user.solve(precond="jacobi")
    assert info["converged"] and np.allclose(x, 0.5)
    # pfv_amg_setup with the sweep selected
    ctx._select_precond("sweep")
    assert ctx.lib.pfv_amg_setup(ctx._h, 0) == 5
    ctx._select_precond("jacobi")
    # before any sweep solve on a transport handle
    q = pa.Upwind(KW).darcy_flux(g, VEL)
    data = data_for(q, None, np.zeros(g.num_faces))
    up = pa.Upwind(KW, library=lib)
    up.discretize(g, data)
    acc = np.ones(g.num_cells)
    up.solve(g, data, accumulation=acc, c_old=acc, method="gmres")
    tctx = up.context(g)
    with pytest.raises(pa.PorefvError) as e:
        tctx.sweep_info()
    assert e.value.status == 4
    up.solve(g, data, accumulation=acc, c_old=acc, precond="sweep")
    assert tctx.sweep_info()["levels"] == 18
    # a new discretization drops the system: the solve is refused as ever
    tctx.upwind_discretize(-q, 1)
    with pytest.raises(RuntimeError):
        tctx.solve(precond="sweep")
    with pytest.raises(pa.PorefvError):
        tctx.transport_advance(np.zeros(g.num_cells), 1, precond="sweep")
    with pytest.raises(ValueError):
        tctx.transport_advance(np.zeros(g.num_cells), 1, precond="amg")
    # a new grid: no order is left
    up.solve(g, data, accumulation=acc, c_old=acc, precond="sweep")
    tctx.sweep_info()
    tctx.set_grid(pa.grid_to_raw(g))
    with pytest.raises(pa.PorefvError) as e:
        tctx.sweep_info()
    assert e.value.status == 4
    # zero diagonal: the existing refusal
    g1 = line_grid(6, 1.0)
    q1 = np.where(g1.face_centers[0] < 0.5, 1.0, -1.0)
    d1 = data_for(q1, None, np.zeros(g1.num_faces))
    up.discretize(g1, d1)
    with pytest.raises(pa.PorefvError) as e:
        up.advance(g1, d1, np.zeros(6), 2, None, precond="sweep")
    assert e.value.status == 5 and "zero diagonal" in e.value.message


def order_follows_the_flux(lib):
    """The order stays while assemblies bring a flux with the same edges, and is rebuilt for one with others."""
    g = tets(3)
    up = pa.Upwind(KW, library=lib)
    q = up.darcy_flux(g, VEL)
    acc = np.ones(g.num_cells)
    data = data_for(q, None, np.zeros(g.num_faces))
    up.discretize(g, data)
    up.advance(g, data, acc, 1, acc, precond="sweep")
    ctx = up.context(g)
    first = ctx.sweep_info()
    assert ctx.stats()["sweep_order_ms"] > 0
    up.advance(g, data, acc, 2, acc, precond="sweep")  # (assembles again, with the same flux)
    assert ctx.stats()["sweep_order_ms"] == 0 and ctx.stats()["sweep_direct_steps"] == 2
    d2 = data_for(-q, None, np.zeros(g.num_faces))
    up.discretize(g, d2)
    up.advance(g, d2, acc, 1, acc, precond="sweep")
    assert ctx.stats()["sweep_order_ms"] > 0
    second = ctx.sweep_info()
    same_order(second, flow_order(g.num_cells, *edges(g, -q)))
    assert not np.array_equal(first["level"], second["level"])


# ---- 7. nothing else moves ----------------------------------------------------------------------------------------------
def nothing_else_moves(lib, n=4):
    g = tets(n)
    _, _, _, _, src = _injection(g)
    up, _, c, info, st, ref, _ = _three_steps(lib, g, np.zeros(g.num_faces), src, precond="jacobi")
    assert info["steps_done"] == 3
    for k in ("sweep_order_ms", "sweep_levels", "sweep_core_cells", "sweep_launches", "sweep_direct_steps",
              "sweep_direct_fallbacks"):
        assert st[k] == 0, k
    import pytest

    with pytest.raises(pa.PorefvError):
        up.context(g).sweep_info()  # (no order was built)
    pr = AD.problem(g)
    ad, data = AD.discretized(lib, g, pr)
    ad.advance(g, data, pr["c0"], 2, pr["acc"], source=pr["src"])
    st = ad.context(g).stats()
    assert st["sweep_order_ms"] == 0 and st["sweep_levels"] == 0
    UP.deterministic(lib, n)
    AD.deterministic(lib, n)
