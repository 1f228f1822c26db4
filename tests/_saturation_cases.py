"""Cases of the saturation step (pfv_transport_advance_nl, ``Upwind.advance_saturation``), shared by the emulation suite
(test_saturation_emulation.py) and the GPU suite (test_gpu_saturation.py): each takes the library to run on.

Judges (they never touch the library): (J1) a damped global Newton solve of ``F(s) = 0`` with scipy's spsolve, ``A``,
``b_ref`` and the upstream rule restated in scipy from ``g.cell_faces`` and ``q`` (_upwind_cases.upwind_numpy),
converged to ``max|ds| <= 1e-14`` and never clipped into [0, 1]; (J2) for the 1-D line, the cell-by-cell recursion with
``scipy.optimize.brentq``.  ``judges_agree_on_the_line`` holds one against the other."""
import ctypes as C
import re

import numpy as np
import pytest
import scipy.optimize as spo
import scipy.sparse as sps
import scipy.sparse.linalg as spla

import porepy_amd as pa
from tests import _upwind_cases as UP
from tests._sweep_cases import VEL, cyclic_field, edges, env, flow_order, rotation
from tests._upwind_cases import KW, data_for, geo, line_grid, tets

INFLOW = 0.85
COREY = dict(s_wr=0.1, s_nr=0.15, n_w=2.0, n_n=2.0, mu_w=1.0, mu_n=5.0)


def corey(n_w=2.0, n_n=2.0):
    return pa.CoreyFractionalFlow(**{**COREY, "n_w": n_w, "n_n": n_n})


def table9():
    return pa.TabulatedFractionalFlow(corey()(np.linspace(0.0, 1.0, 9)))


def flux_and_slope(ff, s):
    """f(s) from the class's numpy curve; f'(s) restated here (one-sided, 0 where the curve is flat)."""
    s = np.asarray(s, dtype=float)
    if isinstance(ff, str):
        return s.copy(), np.ones_like(s)
    if isinstance(ff, pa.TabulatedFractionalFlow):
        v = ff.values
        k = np.clip(np.floor(np.clip(s, 0.0, 1.0) * (v.size - 1)).astype(int), 0, v.size - 2)
        return ff(s), np.where((s >= 0) & (s <= 1), np.diff(v)[k] * (v.size - 1), 0.0)
    span = 1.0 - ff.s_wr - ff.s_nr
    se = (s - ff.s_wr) / span
    inside = (se > 0) & (se < 1)
    x = np.where(inside, se, 0.5)
    lw, ln = x ** ff.n_w / ff.mu_w, (1 - x) ** ff.n_n / ff.mu_n
    dlw, dln = ff.n_w * x ** (ff.n_w - 1) / ff.mu_w, -ff.n_n * (1 - x) ** (ff.n_n - 1) / ff.mu_n
    return ff(s), np.where(inside, (dlw * ln - lw * dln) / (lw + ln) ** 2 / span, 0.0)


def cfl_accumulation(g, q, cfl):
    """acc = max(A_ii) / CFL in every cell"""
    A, _ = scipy_system(g, q, np.zeros(g.num_faces), "linear")
    return np.full(g.num_cells, A.diagonal().max() / cfl)


def scipy_system(g, q, bv, ff, flags=None):
    """A = div diag(q) U and b_ref = div (rhs_neu bc + rhs_dir diag(q) f(bc)) from cell_faces and q alone."""
    is_dir, is_neu = UP.default_flags(g) if flags is None else flags
    mats = UP.upwind_numpy(g, q, is_dir, is_neu)
    div = sps.csr_matrix(g.cell_faces).T.tocsr()
    Q = sps.diags(q)
    fb = flux_and_slope(ff, np.clip(bv, 0.0, 1.0))[0]
    used = np.asarray(abs(mats["rhs_dir"]).sum(axis=1)).ravel() > 0  # (values on the other faces are not read)
    return sps.csr_matrix(div @ Q @ mats["transport"]), div @ (mats["rhs_neu"] @ bv + mats["rhs_dir"] @ (Q @ np.where(used, fb, 0.0)))


def newton_step(A, bref, acc, s_old, ff, source=None, sink=None, tol=1e-14):
    """(J1) one implicit step by damped global Newton, unclipped."""
    src = 0.0 if source is None else source
    M = sps.csr_matrix(A + (0.0 if sink is None else sps.diags(sink)))

    def F(s):
        f, df = flux_and_slope(ff, s)
        return acc * (s - s_old) + M @ f + bref - src, df

    s = s_old.copy()
    r, df = F(s)
    for _ in range(200):
        ds = spla.spsolve((sps.diags(acc) + M @ sps.diags(df)).tocsc(), -r)
        t = 1.0
        while True:
            rn, dfn = F(s + t * ds)
            if np.linalg.norm(rn) <= (1 - 1e-4 * t) * np.linalg.norm(r) or t < 1e-3 or np.abs(t * ds).max() <= 1e-12:
                break
            t *= 0.5
        s, r, df = s + t * ds, rn, dfn
        if np.abs(t * ds).max() <= tol:
            return s
    raise AssertionError("the judge's Newton solve did not converge")


def newton_steps(g, q, bv, acc, s0, ff, n, source=None, sink=None, tol=1e-14):
    A, bref = scipy_system(g, q, bv, ff)
    out = [s0]
    for _ in range(n):
        out.append(newton_step(A, bref, acc, out[-1], ff, source, sink, tol))
    return out


def line_recursion(qv, bv0, acc, s0, ff, n, source=None, sink=None):
    """(J2) the line with q = qv > 0: cell i is one scalar equation given cell i - 1."""
    nc = s0.size
    src = np.zeros(nc) if source is None else source
    snk = np.zeros(nc) if sink is None else sink
    s = s0.copy()
    for _ in range(n):
        new = np.empty(nc)
        up = float(flux_and_slope(ff, np.array([bv0]))[0][0])
        for i in range(nc):
            gi = lambda x: acc[i] * (x - s[i]) + (qv + snk[i]) * float(flux_and_slope(ff, np.array([x]))[0][0]) - qv * up - src[i]  # noqa: E731
            new[i] = spo.brentq(gi, 0.0, 1.0, xtol=1e-16, rtol=8.9e-16)
            up = float(flux_and_slope(ff, new[i:i + 1])[0][0])
        s = new
    return s


def discretized(lib, g, q, bv, bc=None):
    data = data_for(q, bc, bv)
    up = pa.Upwind(KW, library=lib)
    up.discretize(g, data)
    return up, data


def inflow_values(g, value=INFLOW):
    bv = np.zeros(g.num_faces)
    bv[g.get_all_boundary_faces()] = value  # (read on the Dirichlet inflow faces only)
    return bv


def line_problem(with_wells):
    g = line_grid(16, 2.0)
    q = np.ones(g.num_faces)
    bv = np.zeros(g.num_faces)
    bv[0] = INFLOW
    acc = np.full(16, 0.5)  # CFL 2
    source = sink = None
    if with_wells:
        source, sink = np.zeros(16), np.zeros(16)
        source[0], sink[15] = 0.01, 0.5
    return g, q, bv, acc, np.full(16, 0.1), source, sink


# ---- 0. the judges against each other (no library) ---------------------------------------------------------------------
def judges_agree_on_the_line():
    for n_w, n_n in ((2.0, 2.0), (3.0, 1.5)):
        for wells in (False, True):
            g, q, bv, acc, s0, source, sink = line_problem(wells)
            ff = corey(n_w, n_n)
            j1 = newton_steps(g, q, bv, acc, s0, ff, 5, source, sink)[-1]
            j2 = line_recursion(1.0, bv[0], acc, s0, ff, 5, source, sink)
            assert np.abs(j1 - j2).max() <= 1e-13, (n_w, n_n, wells, np.abs(j1 - j2).max())
            assert j2.max() - j2.min() > 0.1  # (a front is there)


# ---- 1. exact against the global Newton solve ---------------------------------------------------------------------------
def exact(lib, n, kind):
    g = tets(n)
    q = pa.Upwind(KW).darcy_flux(g, VEL)
    assert flow_order(g.num_cells, *edges(g, q))["core_cells"] == 0
    ff = corey() if kind == "corey" else table9()
    bv, acc, s0 = inflow_values(g), cfl_accumulation(g, q, 5.0), np.full(g.num_cells, 0.1)
    ref = newton_steps(g, q, bv, acc, s0, ff, 3)[-1]
    up, data = discretized(lib, g, q, bv)
    s, info = up.advance_saturation(g, data, s0, 3, acc, ff, rtol=1e-12)
    st = up.context(g).stats()
    lin, ldata = discretized(lib, g, q, bv)
    lin.advance(g, ldata, s0, 1, acc, precond="sweep")
    single = lin.context(g).stats()
    err = np.abs(s - ref).max()
    print(f"tets({n}), {kind}: max|s - s_J1| = {err:.2e} after 3 steps at CFL 5, relative residual "
          f"{info['rel_residual']:.2e}, {st['sweep_levels']} levels, {st['sweep_launches']} launches")
    assert info["steps_done"] == 3 and info["converged"] and info["iterations"] == 1
    assert st["sweep_core_cells"] == 0 and st["transport_nl_steps"] == 3 and st["transport_nl_core_iterations"] == 0
    assert st["sweep_launches"] == single["sweep_launches"] > 0 and st["sweep_levels"] == single["sweep_levels"]
    assert info["rel_residual"] <= 1e-12
    assert ref.max() - ref.min() > 0.05 and 0 <= s.min() and s.max() <= 1  # (a front, inside the interval)
    assert err <= 1e-12


# ---- 2. the line against its recursion ------------------------------------------------------------------------------------
def line_case(lib, n_w, n_n, wells):
    g, q, bv, acc, s0, source, sink = line_problem(wells)
    ff = corey(n_w, n_n)
    ref = line_recursion(1.0, bv[0], acc, s0, ff, 5, source, sink)
    bc = pa.BoundaryCondition(g, g.get_all_boundary_faces(), ["dir", "dir"])
    up, data = discretized(lib, g, q, bv, bc)
    s, info = up.advance_saturation(g, data, s0, 5, acc, ff, source=source, sink=sink)
    st = up.context(g).stats()
    err = np.abs(s - ref).max()
    print(f"line, Corey {n_w} / {n_n}, wells {wells}: max|s - s_J2| = {err:.2e}")
    assert info["steps_done"] == 5 and st["sweep_levels"] == 16 and st["sweep_core_cells"] == 0
    assert err <= 1e-13
    if wells:  # (both terms act)
        plain = line_recursion(1.0, bv[0], acc, s0, ff, 5)
        assert abs(ref[0] - plain[0]) > 1e-3 and abs(ref[15] - plain[15]) > 1e-3


# ---- 3. the linear kind is the linear step --------------------------------------------------------------------------------
def linear_kind_is_the_linear_step(lib, n=4):
    g = tets(n)
    q = pa.Upwind(KW).darcy_flux(g, VEL)
    bv, acc = inflow_values(g), cfl_accumulation(g, q, 5.0)
    s0 = 0.1 + 0.5 * np.random.default_rng(4).random(g.num_cells)
    src = np.zeros(g.num_cells)
    src[g.num_cells // 2] = 0.01 * acc[0]
    up, data = discretized(lib, g, q, bv)
    s, info = up.advance_saturation(g, data, s0, 3, acc, "linear", source=src)
    c, i1 = up.advance(g, data, s0, 3, acc, source=src, precond="sweep", rtol=1e-13)
    assert info["steps_done"] == 3 and i1["steps_done"] == 3 and up.context(g).stats()["sweep_direct_steps"] == 3
    err = np.abs(s - c).max() / np.abs(c).max()
    print(f"linear kind against advance(precond='sweep'): {err:.2e} of max|c|")
    assert err <= 1e-13


# ---- 4. a cyclic core converges -------------------------------------------------------------------------------------------
def core_problem(which):
    if which == "cyclic12":
        g, q = cyclic_field(12)
        return g, q, 2.0, np.full(g.num_cells, 0.1), 45
    g, q = rotation(8)
    return g, q, 5.0, 0.2 + 0.5 * np.random.default_rng(3).random(g.num_cells), 64


def core_converges(lib, which):
    g, q, cfl, s0, n_core = core_problem(which)
    bv, acc, ff = inflow_values(g), cfl_accumulation(g, q, cfl), corey()
    ref = newton_steps(g, q, bv, acc, s0, ff, 3)[-1]
    up, data = discretized(lib, g, q, bv)
    s, info = up.advance_saturation(g, data, s0, 3, acc, ff, rtol=1e-12)
    st = up.context(g).stats()
    err = np.abs(s - ref).max()
    print(f"{which}: max|s - s_J1| = {err:.2e} after 3 steps at CFL {cfl}, core of {st['sweep_core_cells']} cells, "
          f"{st['transport_nl_core_iterations']} core iterations in all, {info['iterations']} in the last step, "
          f"relative residual {info['rel_residual']:.2e}")
    assert info["steps_done"] == 3 and info["converged"] and info["rel_residual"] <= 1e-12
    assert st["sweep_core_cells"] == n_core and st["transport_nl_core_iterations"] >= info["iterations"] > 0
    assert st["transport_nl_steps"] == 3
    assert err <= 1e-10
    # two iterations are not enough: the call says so and hands the state back untouched
    s2, i2 = up.advance_saturation(g, data, s0, 3, acc, ff, rtol=1e-12, maxit=2, raise_on_fail=False)
    assert i2["steps_done"] == 0 and not i2["converged"] and i2["iterations"] == 2
    assert s2.tobytes() == s0.tobytes()
    with pytest.raises(pa.PorefvError) as e:
        up.advance_saturation(g, data, s0, 3, acc, ff, rtol=1e-12, maxit=2)
    assert e.value.status == 6


# ---- 5. deterministic, and the two launch forms agree ------------------------------------------------------------------------
def deterministic_and_merged(lib, n=6):
    g = tets(n)
    q = pa.Upwind(KW).darcy_flux(g, VEL)
    bv, acc, s0, ff = inflow_values(g), cfl_accumulation(g, q, 5.0), np.full(g.num_cells, 0.1), corey()
    runs = []
    for environment in ({}, {}, {"PFV_SWEEP_MERGE": 0}):
        with env(**environment):
            up, data = discretized(lib, g, q, bv)
            s, info = up.advance_saturation(g, data, s0, 3, acc, ff)
            st = up.context(g).stats()
        assert info["steps_done"] == 3
        runs.append((s, st["sweep_launches"], st["sweep_levels"]))
    print("launches per sweep (merged, merged, one per level):", [r[1] for r in runs])
    assert runs[1][0].tobytes() == runs[0][0].tobytes()
    assert runs[2][0].tobytes() == runs[0][0].tobytes()
    assert runs[2][1] == runs[2][2] and runs[0][1] < runs[2][1]
    g, q, cfl, s0, _ = core_problem("cyclic12")
    bv, acc = inflow_values(g), cfl_accumulation(g, q, cfl)
    both = []
    for _ in range(2):
        up, data = discretized(lib, g, q, bv)
        both.append(up.advance_saturation(g, data, s0, 3, acc, ff)[0])
    assert both[0].tobytes() == both[1].tobytes()


# ---- 6. a step that leaves [0, 1] -----------------------------------------------------------------------------------------
def leaves_the_interval(lib):
    g, q = cyclic_field(12)  # (not solenoidal)
    bv, acc, s0, ff = inflow_values(g), cfl_accumulation(g, q, 5.0), np.full(g.num_cells, 0.1), corey()
    j = newton_steps(g, q, bv, acc, s0, ff, 2)
    assert 0 <= j[1].min() and j[1].max() <= 1
    assert j[2].max() > 1 + 1e-3, j[2].max()  # the judge, unclipped, leaves the interval in the second step
    assert np.abs(j[2] - 1).min() > 1e-9 and j[2].min() > 1e-9  # (no cell on the edge: the lowest one is well defined)
    lowest = int(np.flatnonzero(j[2] > 1).min())
    up, data = discretized(lib, g, q, bv)
    with pytest.raises(ValueError, match=rf"step 1 leaves \[0, 1\]: no root in cell {lowest}$") as e:
        up.advance_saturation(g, data, s0, 3, acc, ff)
    print(f"second step at CFL 5: the judge reaches {j[2].max():.4f}, lowest cell above 1: {lowest}")
    assert e.value.info["steps_done"] == 1
    assert np.abs(e.value.state - j[1]).max() <= 1e-10
    assert up.context(g).stats()["transport_nl_steps"] == 1


# ---- 7. errors ------------------------------------------------------------------------------------------------------------
def errors(lib):
    g = geo(pa.CartGrid([4, 3], [4.0, 3.0]))
    nc, nf = g.num_cells, g.num_faces
    bf = g.get_all_boundary_faces()
    q = pa.Upwind(KW).darcy_flux(g, [1.0, 0.5, 0.0])
    cfd = sps.csc_matrix(g.cell_faces)
    inflow = np.array([f for f in bf if (q[f] >= 0) != (sps.find(cfd[f])[2][0] > 0)])
    outflow = np.setdiff1d(bf, inflow)
    bv, acc, s0, ff = inflow_values(g), cfl_accumulation(g, q, 2.0), np.full(nc, 0.1), corey()
    ref = newton_steps(g, q, bv, acc, s0, "linear", 2)[-1]

    def refused(up, data, status, text, *, s=s0, a=acc, f=ff, **kw):
        """the call is refused with that status and text; afterwards the handle serves a correct advance"""
        ctx = up.context(g)
        pd = data[pa.PARAMETERS][KW]
        kind, par = (0, ()) if isinstance(f, str) else f if isinstance(f, tuple) else (f.kind, f.params)
        with pytest.raises(pa.PorefvError) as e:
            ctx.transport_advance_nl(s, 1, a, pd["bc_values"], kind, par, q=pd.get("darcy_flux"), **kw)
        assert e.value.status == status and text in e.value.message, (e.value.status, e.value.message)
        if status == 4:
            with pytest.raises(ValueError, match=re.escape(text)):
                up.advance_saturation(g, data, s, 1, a, f if not isinstance(f, tuple) else _Raw(*f), **kw)
        good = data_for(q, None, bv)
        up.discretize(g, good)
        c, info = up.advance(g, good, s0, 2, acc, precond="sweep")
        assert info["steps_done"] == 2 and np.abs(c - ref).max() <= 1e-12

    up = pa.Upwind(KW, library=lib)
    data = data_for(q, None, bv)
    # call order
    refused(up, data, 4, "pfv_upwind_discretize first")
    d2 = data_for(q, None, bv, k=2)
    up.discretize(g, d2)
    refused(up, d2, 4, "num_components = 1")
    # the flux function
    up.discretize(g, data)
    refused(up, data, 4, "unknown flux function kind 7", f=(7, ()))
    refused(up, data, 4, "n_params = 5", f=(1, ff.params[:5]))
    refused(up, data, 4, "n_params = 1", f=(0, [1.0]))
    for bad, text in ((dict(s_wr=-0.1), "s_wr (index 0)"), (dict(s_nr=-0.1), "s_nr (index 1)"),
                      (dict(s_wr=0.5, s_nr=0.5), "s_wr + s_nr"), (dict(n_w=0.0), "n_w (index 2)"),
                      (dict(n_n=-1.0), "n_n (index 3)"), (dict(mu_w=0.0), "mu_w (index 4)"),
                      (dict(mu_n=-2.0), "mu_n (index 5)"), (dict(mu_n=np.nan), "mu_n (index 5)")):
        refused(up, data, 4, text, f=pa.CoreyFractionalFlow(**{**COREY, **bad}))
    refused(up, data, 4, "decreases at value 3", f=pa.TabulatedFractionalFlow([0.0, 0.2, 0.5, 0.4, 1.0]))
    refused(up, data, 4, "value 2 is not finite", f=pa.TabulatedFractionalFlow([0.0, 0.2, np.inf, 1.0]))
    refused(up, data, 4, "n_params = 1)", f=pa.TabulatedFractionalFlow([0.5]))
    refused(up, data, 4, "n_params = 1025", f=pa.TabulatedFractionalFlow(np.linspace(0, 1, 1025)))
    # the arrays, each with the lowest offender
    a = acc.copy()
    a[[5, 9]] = [0.0, -1.0]
    refused(up, data, 4, "accumulation must be positive: cell 5", a=a)
    a = acc.copy()
    a[7] = np.nan
    refused(up, data, 4, "accumulation must be positive: cell 7", a=a)
    k = np.zeros(nc)
    k[[3, 8]] = -1e-3
    refused(up, data, 4, "negative sink in cell 3", sink=k)
    s = s0.copy()
    s[[4, 6]] = [1.0 + 1e-12, -0.5]
    refused(up, data, 4, "s outside [0, 1] in cell 4", s=s)
    b2 = bv.copy()
    b2[outflow] = 7.0  # values on outflow faces are not read
    up.discretize(g, data_for(q, None, b2))
    got, info = up.advance_saturation(g, data_for(q, None, b2), s0, 1, acc, ff)
    assert info["steps_done"] == 1
    b2[inflow[[1, 2]]] = [1.5, -0.5]
    refused(up, data_for(q, None, b2), 4, f"Dirichlet inflow value outside [0, 1] on face {inflow[[1, 2]].min()}")
    # the inflow-face rule: a Robin face that has outflow in the discretization, inflow in the flux of the call
    kinds = np.array(["dir"] * bf.size, dtype=object)
    kinds[np.isin(bf, outflow[:2])] = "rob"
    rob = pa.BoundaryCondition(g, bf, list(kinds))
    up.discretize(g, data_for(q, rob, bv))
    refused(up, data_for(-q, rob, bv), 4, f"face {outflow[:2].min()}")
    # periodic grids, conditions per sub-face
    gp = geo(pa.CartGrid([3, 3], [1.0, 1.0]))
    gp.periodic_face_map = np.vstack([np.flatnonzero(np.isclose(gp.face_centers[0], 0.0)),
                                      np.flatnonzero(np.isclose(gp.face_centers[0], 1.0))])
    with pytest.raises(pa.PorefvError) as e:
        pa.Upwind(KW, library=lib).advance_saturation(gp, data_for(np.ones(gp.num_faces), None, np.zeros(gp.num_faces)),
                                                      np.zeros(9), 1, np.ones(9), ff)
    assert e.value.status == 5
    fdata, _ = UP.flow_problem(g, np.random.default_rng(23))
    mp = pa.Mpfa("flow", library=lib)
    mp.discretize(g, fdata)
    ups = pa.Upwind(KW, library=lib, flow=mp)
    ups.discretize(g, data)
    ctx = mp.context(g)
    ctx.set_subface_bc(np.ones(ctx.nsf, dtype=np.uint8))  # (Dirichlet on every sub-face; only the switch matters here)
    with pytest.raises(pa.PorefvError) as e:
        ups.advance_saturation(g, data, s0, 1, acc, ff)
    assert e.value.status == 5 and "sub-face" in e.value.message
    ctx.set_subface_bc(None)
    got, info = ups.advance_saturation(g, data, s0, 1, acc, ff)
    assert info["steps_done"] == 1


class _Raw(pa.TabulatedFractionalFlow):
    """a (kind, parameters) pair no class would produce, for the checks of the C entry point through ``Upwind``"""

    def __init__(self, kind, params):
        self.kind, self.values = kind, np.array(params, dtype=np.float64).ravel()


# ---- 8. lifetime ----------------------------------------------------------------------------------------------------------
def lifetime(lib, n=4):
    g = tets(n)
    q = pa.Upwind(KW).darcy_flux(g, VEL)
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)
    bv, acc, s0, ff = inflow_values(g), cfl_accumulation(g, q, 5.0), np.full(g.num_cells, 0.1), corey()
    up, data = discretized(lib, g, q, bv, bc)
    ctx = up.context(g)
    # no assembly is needed, and none is left behind
    s, info = up.advance_saturation(g, data, s0, 2, acc, ff)
    assert info["steps_done"] == 2 and ctx.stats()["sweep_order_ms"] > 0
    assert ctx.active_size() == 0
    with pytest.raises(RuntimeError):
        ctx.solve()
    with pytest.raises(pa.PorefvError):
        ctx.transport_advance(np.zeros(g.num_cells), 1)
    # the same flux again: the order is kept; other edges: rebuilt
    up.advance_saturation(g, data, s0, 1, acc, ff)
    assert ctx.stats()["sweep_order_ms"] == 0
    first = ctx.sweep_info()
    d2 = data_for(-q, bc, bv)
    up.discretize(g, d2)
    up.advance_saturation(g, d2, s0, 1, acc, ff)
    assert ctx.stats()["sweep_order_ms"] > 0
    assert not np.array_equal(first["level"], ctx.sweep_info()["level"])
    # a selected preconditioner stays selected: the C call below selects nothing itself
    jac, jdata = discretized(lib, g, q, bv, bc)
    c1, i1 = jac.advance(g, jdata, s0, 1, acc, method="gmres")  # selects "jacobi"
    jac.advance_saturation(g, jdata, s0, 1, acc, ff)
    jctx = jac.context(g)
    jac._assemble(g, jdata, acc, None, None)
    c2, done, last = s0.copy(), C.c_int32(0), pa._lib.SolveInfo()
    st = jctx.lib.pfv_transport_advance(jctx._h, 1, pa._lib.SOLVE_GMRES, 1e-12, 20000, pa._lib._ptr(c2, pa._lib._dp),
                                        C.byref(done), C.byref(last))
    assert st == 0 and done.value == 1 and last.iterations == i1["iterations"] > 1
    assert c2.tobytes() == c1.tobytes() and jctx.stats()["sweep_direct_steps"] == 0


def flow_system_is_untouched(lib, n=3):
    """Upwind(flow=mpfa) shares the handle: after the saturation call the flow system assembles and solves to the bits
    of a handle that never saw it (the model: _multi_cases.flow_system_is_untouched)."""
    def flow(with_transport):
        g = tets(n)
        fdata, _ = UP.flow_problem(g, np.random.default_rng(23))
        mp = pa.Mpfa("flow", library=lib)
        mp.discretize(g, fdata)
        p, _ = mp.solve(g, fdata, rtol=1e-12)
        if with_transport:
            mp.darcy_flux(g, fdata, p, resident=True)
            up = pa.Upwind(KW, library=lib, flow=mp)
            assert up.context(g) is mp.context(g)
            tdata = pa.initialize_data({}, KW, {"bc_values": inflow_values(g)})
            up.discretize(g, tdata)
            qd = np.abs(mp.context(g).resident_flux())
            acc = np.full(g.num_cells, 4 * qd.max())
            s, info = up.advance_saturation(g, tdata, np.full(g.num_cells, 0.1), 2, acc, corey(), maxit=2000)
            assert info["steps_done"] == 2 and s.max() > 0.1 + 1e-6
        A, b = mp.assemble_matrix_rhs(g, fdata)
        x, info = mp.solve(g, fdata, rtol=1e-12)
        return p, A, b, x, info["iterations"], mp.context(g).matrix(pa._lib.MAT_FLUX)

    p1, A1, b1, x1, it1, F1 = flow(True)
    p2, A2, b2, x2, it2, F2 = flow(False)
    UP.same_csr(A1, A2, "A")
    UP.same_csr(F1, F2, "flux")
    assert p1.tobytes() == p2.tobytes() and np.asarray(b1).tobytes() == np.asarray(b2).tobytes()
    assert x1.tobytes() == x2.tobytes() and it1 == it2
