"""Cases of the saturation step with phase-carried components (pfv_transport_advance_nl_multi,
``Upwind.advance_saturation_components``), shared by the emulation suite (test_satcomp_emulation.py) and the GPU suite
(test_gpu_satcomp.py): each takes the library to run on.

Judges (they never touch the library).  Saturation: ``newton_steps`` of _saturation_cases (J1), per step.  Component a,
given the judge's saturations of the step: scipy's spsolve of ``diag(acc s_new + ads_a) + (A + diag(sink)) diag(f(s_new))``
against ``(acc s_old + ads_a) c_old - b_ref_a + src_a``, with ``b_ref_a = div (rhs_neu cbc_a + rhs_dir diag(q) (f(bc) o
cbc_a))`` restated in scipy from ``upwind_numpy``.  On the 1-D line also the cell-by-cell recursion: ``brentq`` for ``s``,
one division for ``c``.  ``judges_agree_on_the_line`` holds one against the other.

BOUNDS holds, per case, ten times the largest error the host-emulation build showed against the judge, rounded up to a
power of ten (the factor covers the different multiply-add contraction of the two builds), capped at 1e-9 (1e-8 for
the cyclic cores).  The error is ``max|c_a - c_judge_a| / max|c_judge_a|``, the largest over the components."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.optimize as spo
import scipy.sparse as sps
import scipy.sparse.linalg as spla

import porepy_amd as pa
from tests import _upwind_cases as UP
from tests._saturation_cases import (cfl_accumulation, core_problem, corey, discretized, flux_and_slope,
                                     inflow_values, line_problem, newton_steps, scipy_system, table9)
from tests._sweep_cases import VEL, cyclic_field, edges, env, flow_order
from tests._upwind_cases import KW, tets

S_BOUND = 1e-12  # the saturation against J1 (the bound of the saturation step's own suite)
BOUNDS = {                 # largest error of the emulation build -> bound
    "judge": 1e-13,        # tets(3), tets(4): Corey and table, k = 1, 3, 4, 5: 3.41e-15
    "line": 1e-13,         # the line against its recursion, k = 2: 5.36e-15
    "line64": 1e-13,       # the line, k = 64, against spsolve: 2.95e-15
    "marking": 1e-13,      # c stays 1: 3.11e-15
    "linear": 1e-14,       # against advance_components(precond="sweep"): 7.78e-16
    "cyclic12": 1e-11,     # the cyclic cores, k = 2: 1.44e-13
    "rotation8": 1e-11,    # 8.43e-13
    "cyclic12-k64": 1e-10,  # not from a run: the project's bound for a cyclic core stopped at rtol = 1e-12 (err_s below)
    "refused": 1e-10,      # the state handed back by the refused step (a core case): 2.03e-12
}


def rel_err(c, ref):
    return max(np.abs(c[a] - ref[a]).max() / np.abs(ref[a]).max() for a in range(ref.shape[0]))


# ---- the judges -----------------------------------------------------------------------------------------------------------
def component_bref(g, q, bv, cbv, ff):
    """b_ref_a of every component, from cell_faces and q alone"""
    is_dir, is_neu = UP.default_flags(g)
    mats = UP.upwind_numpy(g, q, is_dir, is_neu)
    div = sps.csr_matrix(g.cell_faces).T.tocsr()
    Q = sps.diags(q)
    fb = flux_and_slope(ff, np.clip(bv, 0.0, 1.0))[0]
    used = np.asarray(abs(mats["rhs_dir"]).sum(axis=1)).ravel() > 0  # (values on the other faces are not read)
    return np.array([div @ (mats["rhs_neu"] @ cb + mats["rhs_dir"] @ (Q @ np.where(used, fb * cb, 0.0))) for cb in cbv])


def component_steps(g, q, bv, cbv, acc, ff, s_traj, c0, sorption=None, c_source=None, sink=None):
    """the components along the judge's saturations s_traj[0], s_traj[1], ...: one spsolve per component and step"""
    k, nc = c0.shape
    A, _ = scipy_system(g, q, bv, ff)
    M = sps.csr_matrix(A + (0.0 if sink is None else sps.diags(sink)))
    bref = component_bref(g, q, bv, cbv, ff)
    ads = np.zeros((k, nc)) if sorption is None else sorption
    src = np.zeros((k, nc)) if c_source is None else c_source
    out = [c0]
    for s_old, s_new in zip(s_traj[:-1], s_traj[1:]):
        T = M @ sps.diags(flux_and_slope(ff, s_new)[0])
        out.append(np.array([spla.spsolve((sps.diags(acc * s_new + ads[a]) + T).tocsc(),
                                          (acc * s_old + ads[a]) * out[-1][a] - bref[a] + src[a]) for a in range(k)]))
    return out


def line_recursion(qv, bv0, cb0, acc, s0, c0, ff, n, source=None, sink=None, sorption=None, c_source=None):
    """the line with q = qv > 0, cell by cell: brentq for s_i given cell i - 1, then one division per component"""
    k, nc = c0.shape
    f = lambda x: float(flux_and_slope(ff, np.array([x]))[0][0])  # noqa: E731
    src = np.zeros(nc) if source is None else source
    snk = np.zeros(nc) if sink is None else sink
    ads = np.zeros((k, nc)) if sorption is None else sorption
    csrc = np.zeros((k, nc)) if c_source is None else c_source
    s, c = s0.copy(), c0.copy()
    for _ in range(n):
        s_new, c_new = np.empty(nc), np.empty((k, nc))
        up_phi = f(bv0)
        up_psi = up_phi * np.asarray(cb0, dtype=float)
        for i in range(nc):
            gi = lambda x: acc[i] * (x - s[i]) + (qv + snk[i]) * f(x) - qv * up_phi - src[i]  # noqa: E731
            s_new[i] = spo.brentq(gi, 0.0, 1.0, xtol=1e-16, rtol=8.9e-16)
            up_phi = f(s_new[i])
            d = acc[i] * s_new[i] + ads[:, i] + (qv + snk[i]) * up_phi
            c_new[:, i] = ((acc[i] * s[i] + ads[:, i]) * c[:, i] + qv * up_psi + csrc[:, i]) / d
            up_psi = up_phi * c_new[:, i]
        s, c = s_new, c_new
    return s, c


def line_components(k, wells, sorb, seed=11):
    """k components on line_problem: own inflow concentrations, a random start, sorption on component 0, a component
    source in cell 3 of the last one"""
    g, q, bv, acc, s0, source, sink = line_problem(wells)
    rng = np.random.default_rng(seed)
    cbv = np.zeros((k, g.num_faces))
    cbv[:, 0] = 0.5 + 0.25 * np.arange(k)
    c0 = 0.2 + rng.random((k, 16))
    ads = None
    if sorb:
        ads = np.zeros((k, 16))
        ads[0] = 0.3 * acc
    csrc = np.zeros((k, 16))
    csrc[k - 1, 3] = 0.02
    return g, q, bv, acc, s0, source, sink, cbv, c0, ads, csrc


def judges_agree_on_the_line():
    for n_w, n_n in ((2.0, 2.0), (3.0, 1.5)):
        for wells in (False, True):
            g, q, bv, acc, s0, source, sink, cbv, c0, ads, csrc = line_components(2, wells, True)
            ff = corey(n_w, n_n)
            traj = newton_steps(g, q, bv, acc, s0, ff, 5, source, sink)
            j1 = component_steps(g, q, bv, cbv, acc, ff, traj, c0, ads, csrc, sink)[-1]
            s2, j2 = line_recursion(1.0, bv[0], cbv[:, 0], acc, s0, c0, ff, 5, source, sink, ads, csrc)
            assert np.abs(traj[-1] - s2).max() <= 1e-13
            assert rel_err(j1, j2) <= 1e-12, (n_w, n_n, wells, rel_err(j1, j2))
            assert np.abs(j2[0] - j2[1]).max() > 1e-2  # (the components differ)


# ---- 1. against the judge -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tets_problem(n, kind):
    g = tets(n)
    q = pa.Upwind(KW).darcy_flux(g, VEL)
    assert flow_order(g.num_cells, *edges(g, q))["core_cells"] == 0
    ff = corey() if kind == "corey" else "linear" if kind == "linear" else table9()
    bv, acc, s0 = inflow_values(g), cfl_accumulation(g, q, 5.0), np.full(g.num_cells, 0.1)
    traj = newton_steps(g, q, bv, acc, s0, ff, 3)
    return g, q, ff, bv, acc, s0, traj


def tets_components(g, acc, k, seed=7):
    """distinct inflow concentrations, a random start; component 0 sorbs, the last one has a source cell"""
    nc = g.num_cells
    rng = np.random.default_rng(seed)
    cbv = np.zeros((k, g.num_faces))
    cbv[:, g.get_all_boundary_faces()] = (0.5 * (1 + np.arange(k)))[:, None]
    c0 = 0.2 + rng.random((k, nc))
    ads = np.zeros((k, nc))
    ads[0] = 0.3 * acc
    csrc = np.zeros((k, nc))
    csrc[k - 1, nc // 2] = 0.01 * acc[0]
    return cbv, c0, ads, csrc


def against_judge(lib, n, kind, k):
    g, q, ff, bv, acc, s0, traj = _tets_problem(n, kind)
    cbv, c0, ads, csrc = tets_components(g, acc, k)
    ref = component_steps(g, q, bv, cbv, acc, ff, traj, c0, ads, csrc)[-1]
    up, data = discretized(lib, g, q, bv)
    s, c, info = up.advance_saturation_components(g, data, s0, c0, 3, acc, ff, c_bc_values=cbv, sorption=ads,
                                                  c_source=csrc, rtol=1e-12)
    st = up.context(g).stats()
    err_s, err = np.abs(s - traj[-1]).max(), rel_err(c, ref)
    print(f"tets({n}), {kind}, k = {k}: max|s - s_J1| = {err_s:.2e}, components {err:.2e} of max|c_judge| after 3 steps "
          f"at CFL 5; {st['sweep_levels']} levels, {st['sweep_launches']} launches")
    assert c.shape == (k, g.num_cells) and info["steps_done"] == 3 and info["converged"] and all(info["c_converged"])
    assert st["transport_nl_components"] == k and st["transport_nl_steps"] == 3 and st["sweep_core_cells"] == 0
    assert max(info["c_rel_residual"]) <= 1e-12 and info["rel_residual"] <= 1e-12
    assert np.abs(ref[0] - c0[0]).max() > 1e-2  # (something moved)
    assert err_s <= S_BOUND
    assert err <= BOUNDS["judge"]


# ---- 2. the line against its recursion -----------------------------------------------------------------------------------
def line_case(lib, n_w, n_n, wells, sorb):
    g, q, bv, acc, s0, source, sink, cbv, c0, ads, csrc = line_components(2, wells, sorb)
    ff = corey(n_w, n_n)
    s_ref, ref = line_recursion(1.0, bv[0], cbv[:, 0], acc, s0, c0, ff, 5, source, sink, ads, csrc)
    bc = pa.BoundaryCondition(g, g.get_all_boundary_faces(), ["dir", "dir"])
    up, data = discretized(lib, g, q, bv, bc)
    s, c, info = up.advance_saturation_components(g, data, s0, c0, 5, acc, ff, c_bc_values=cbv, sorption=ads,
                                                  source=source, sink=sink, c_source=csrc)
    st = up.context(g).stats()
    err_s, err = np.abs(s - s_ref).max(), rel_err(c, ref)
    print(f"line, Corey {n_w} / {n_n}, wells {wells}, sorption {sorb}: max|s - s_J2| = {err_s:.2e}, components {err:.2e}")
    assert info["steps_done"] == 5 and st["sweep_levels"] == 16 and st["sweep_core_cells"] == 0
    assert err_s <= 1e-13
    assert err <= BOUNDS["line"]
    if sorb:  # (the retardation is there)
        plain = line_recursion(1.0, bv[0], cbv[:, 0], acc, s0, c0, ff, 5, source, sink, None, csrc)[1]
        assert np.abs(plain[0] - ref[0]).max() > 1e-3 and np.abs(plain[1] - ref[1]).max() == 0.0


def line_k64(lib):
    g, q, bv, acc, s0, source, sink, cbv, c0, ads, csrc = line_components(64, True, True)
    ff = corey()
    traj = newton_steps(g, q, bv, acc, s0, ff, 5, source, sink)
    ref = component_steps(g, q, bv, cbv, acc, ff, traj, c0, ads, csrc, sink)[-1]
    bc = pa.BoundaryCondition(g, g.get_all_boundary_faces(), ["dir", "dir"])
    up, data = discretized(lib, g, q, bv, bc)
    s, c, info = up.advance_saturation_components(g, data, s0, c0, 5, acc, ff, c_bc_values=cbv, sorption=ads,
                                                  source=source, sink=sink, c_source=csrc)
    err = rel_err(c, ref)
    print(f"line, k = 64: components {err:.2e} of max|c_judge|")
    assert info["steps_done"] == 5 and len(info["c_converged"]) == 64 and all(info["c_converged"])
    assert up.context(g).stats()["transport_nl_components"] == 64
    assert np.abs(s - traj[-1]).max() <= 1e-13
    assert err <= BOUNDS["line64"]


# ---- 3. a component that marks the water is the water ----------------------------------------------------------------------
def water_marking(lib, where):
    """c0 = 1, cbc = 1 on the inflow, c_source = source, no sorption: the component's equation is the saturation's, so
    c stays 1 -- which needs the right o_i, the right s_old weight and the right boundary term at once."""
    if where == "line":
        g, q, bv, acc, s0, source, sink = line_problem(True)
        bc, n, ff = pa.BoundaryCondition(g, g.get_all_boundary_faces(), ["dir", "dir"]), 5, corey()
    else:
        g, q, ff, bv, acc, s0, _ = _tets_problem(4, "corey")
        bc, n = None, 3
        source, sink = np.zeros(g.num_cells), np.zeros(g.num_cells)
        source[g.num_cells // 3], sink[2 * g.num_cells // 3] = 0.02 * acc[0], 0.5 * acc[0]
    k = 2
    cbv = np.ones((k, g.num_faces))
    up, data = discretized(lib, g, q, bv, bc)
    s, c, info = up.advance_saturation_components(g, data, s0, np.ones((k, g.num_cells)), n, acc, ff, c_bc_values=cbv,
                                                  source=source, sink=sink, c_source=source)
    err = np.abs(c - 1.0).max()
    print(f"water marking, {where}: max|c - 1| = {err:.2e}, s in [{s.min():.3f}, {s.max():.3f}]")
    assert info["steps_done"] == n and s.max() - s.min() > 0.05
    assert err <= BOUNDS["marking"]


# ---- 4. with f(s) = s and a constant saturation the step is the linear multi-component step ---------------------------------
def reduces_to_linear_components(lib, k=3, s_const=0.6):
    g, q, _, _, acc, _, _ = _tets_problem(4, "linear")
    nc = g.num_cells
    bv, s0 = inflow_values(g, s_const), np.full(nc, s_const)
    traj = newton_steps(g, q, bv, acc, s0, "linear", 3)
    assert all(0.0 <= t.min() and t.max() <= 1.0 and np.abs(t - s_const).max() <= 1e-12 for t in traj)  # (the judge stays inside)
    cbv, c0, ads, csrc = tets_components(g, acc, k)
    up, data = discretized(lib, g, q, bv)
    s, c, info = up.advance_saturation_components(g, data, s0, c0, 3, acc, "linear", c_bc_values=cbv, sorption=ads,
                                                  c_source=csrc)
    lin, ldata = discretized(lib, g, q, bv)
    want, linfo = lin.advance_components(g, ldata, c0, 3, acc[None, :] + ads / s_const, bc_values=cbv,
                                         source=csrc / s_const, precond="sweep", rtol=1e-13)
    err = rel_err(c, want)
    print(f"linear kind at s = {s_const}: max|s - {s_const}| = {np.abs(s - s_const).max():.2e}, components against "
          f"advance_components {err:.2e}")
    assert info["steps_done"] == 3 and linfo["steps_done"] == 3
    assert lin.context(g).stats()["transport_multi_direct_steps"] == 3
    assert np.abs(s - s_const).max() <= S_BOUND
    assert err <= BOUNDS["linear"]


# ---- 5. the saturation is that of advance_saturation, to the bit ------------------------------------------------------------
def _core_setup(which, k=2):
    g, q, cfl, s0, n_core = core_problem(which)
    bv, acc = inflow_values(g), cfl_accumulation(g, q, cfl)
    rng = np.random.default_rng(5)
    cbv = np.zeros((k, g.num_faces))
    cbv[:, g.get_all_boundary_faces()] = (0.5 + np.arange(k))[:, None]
    c0 = 0.2 + rng.random((k, g.num_cells))
    ads = np.zeros((k, g.num_cells))
    ads[0] = 0.3 * acc
    return g, q, bv, acc, s0, n_core, cbv, c0, ads


def saturation_unchanged(lib, which):
    if which == "tets4":
        g, q, ff, bv, acc, s0, _ = _tets_problem(4, "corey")
        cbv, c0, ads, csrc = tets_components(g, acc, 3)
    else:
        g, q, bv, acc, s0, _, cbv, c0, ads = _core_setup(which)
        ff, csrc = corey(), None
    up, data = discretized(lib, g, q, bv)
    s, c, info = up.advance_saturation_components(g, data, s0, c0, 3, acc, ff, c_bc_values=cbv, sorption=ads, c_source=csrc)
    launches = up.context(g).stats()["sweep_launches"]
    alone, adata = discretized(lib, g, q, bv)
    want, winfo = alone.advance_saturation(g, adata, s0, 3, acc, ff)
    assert info["steps_done"] == 3 and winfo["steps_done"] == 3
    assert s.tobytes() == want.tobytes()
    if which == "tets4":  # (with a core the components can ask for further iterations, which are launches)
        assert launches == alone.context(g).stats()["sweep_launches"] > 0
        assert info["iterations"] == 1


# ---- 6. deterministic; the launch forms agree ------------------------------------------------------------------------------
def plan_launches(sizes, rows):
    """launches of the plan: consecutive levels of at most `rows` rows share one"""
    n, prev_small = 0, False
    for m in sizes:
        small = m <= rows
        n += 0 if small and prev_small else 1
        prev_small = small
    return n


def launch_forms(lib, k=3, rows=24):
    g, q, ff, bv, acc, s0, _ = _tets_problem(4, "corey")
    cbv, c0, ads, csrc = tets_components(g, acc, k)
    order = flow_order(g.num_cells, *edges(g, q))
    sizes = np.bincount(order["level"], minlength=order["levels"])
    want = plan_launches(sizes, rows)
    assert plan_launches(sizes, 512) < want < order["levels"]  # (`rows` mixes single levels and runs)
    assert any(a <= rows and b <= rows for a, b in zip(sizes[:-1], sizes[1:])) and (sizes > rows).any()
    runs = []
    for environment in ({}, {}, {"PFV_SWEEP_MERGE": 0}, {"PFV_SWEEP_MERGE_ROWS": rows}):
        with env(**environment):
            up, data = discretized(lib, g, q, bv)
            s, c, info = up.advance_saturation_components(g, data, s0, c0, 3, acc, ff, c_bc_values=cbv, sorption=ads,
                                                          c_source=csrc)
            st = up.context(g).stats()
            alone, adata = discretized(lib, g, q, bv)
            alone.advance_saturation(g, adata, s0, 3, acc, ff)
            assert st["sweep_launches"] == alone.context(g).stats()["sweep_launches"]
        assert info["steps_done"] == 3
        runs.append((s, c, st["sweep_launches"], st["sweep_levels"]))
    print("launches per sweep (merged, merged, one per level, mixed):", [r[2] for r in runs])
    for r in runs[1:]:
        assert r[0].tobytes() == runs[0][0].tobytes() and r[1].tobytes() == runs[0][1].tobytes()
    assert runs[2][2] == runs[2][3] == order["levels"] and runs[0][2] == plan_launches(sizes, 512)
    assert runs[3][2] == want


# ---- 7. a cyclic core iterates s and c jointly -------------------------------------------------------------------------------
def core_case(lib, which):
    """which: the core, or "<core>-k<k>" for k components (k = 64: one slot per component in the core rows' norms)"""
    core, _, kk = which.partition("-k")
    g, q, bv, acc, s0, n_core, cbv, c0, ads = _core_setup(core, int(kk or 2))
    ff = corey()
    traj = newton_steps(g, q, bv, acc, s0, ff, 3)
    ref = component_steps(g, q, bv, cbv, acc, ff, traj, c0, ads)[-1]
    up, data = discretized(lib, g, q, bv)
    s, c, info = up.advance_saturation_components(g, data, s0, c0, 3, acc, ff, c_bc_values=cbv, sorption=ads, rtol=1e-12)
    st = up.context(g).stats()
    err_s, err = np.abs(s - traj[-1]).max(), rel_err(c, ref)
    print(f"{which}: max|s - s_J1| = {err_s:.2e}, components {err:.2e} of max|c_judge|; core of {st['sweep_core_cells']} "
          f"cells, {st['transport_nl_core_iterations']} core iterations in all, relative residuals "
          f"{info['rel_residual']:.2e} / {max(info['c_rel_residual']):.2e}")
    assert info["steps_done"] == 3 and info["converged"] and all(info["c_converged"])
    assert st["sweep_core_cells"] == n_core and st["transport_nl_core_iterations"] >= info["iterations"] > 0
    assert info["rel_residual"] <= 1e-12 and max(info["c_rel_residual"]) <= 1e-12
    assert err_s <= 1e-10  # (the bound of the saturation step's core cases)
    assert err <= BOUNDS[which]
    # two iterations are not enough: the call says so and hands both states back untouched
    s2, c2, i2 = up.advance_saturation_components(g, data, s0, c0, 3, acc, ff, c_bc_values=cbv, sorption=ads, maxit=2,
                                                  raise_on_fail=False)
    assert i2["steps_done"] == 0 and not i2["converged"] and i2["iterations"] == 2
    assert s2.tobytes() == s0.tobytes() and c2.tobytes() == c0.tobytes()


# ---- 8. refusals and errors -------------------------------------------------------------------------------------------------
def refused_step(lib):
    g, q = cyclic_field(12)  # (not solenoidal: at CFL 5 the second step leaves [0, 1])
    bv, acc, s0, ff = inflow_values(g), cfl_accumulation(g, q, 5.0), np.full(g.num_cells, 0.1), corey()
    _, _, _, _, _, _, cbv, c0, _ = _core_setup("cyclic12")
    ads = np.zeros_like(c0)
    ads[0] = 0.3 * acc
    j = newton_steps(g, q, bv, acc, s0, ff, 2)
    assert 0 <= j[1].min() and j[1].max() <= 1 and j[2].max() > 1 + 1e-3
    assert int(np.flatnonzero(j[2] > 1).min()) == 86
    ref = component_steps(g, q, bv, cbv, acc, ff, j[:2], c0, ads)[-1]
    up, data = discretized(lib, g, q, bv)
    with pytest.raises(ValueError, match=r"step 1 leaves \[0, 1\]: no root in cell 86$") as e:
        up.advance_saturation_components(g, data, s0, c0, 3, acc, ff, c_bc_values=cbv, sorption=ads)
    s, c = e.value.state
    err = rel_err(c, ref)
    print(f"refused second step: the state handed back is the judge's first step to {np.abs(s - j[1]).max():.2e} (s), "
          f"{err:.2e} (components)")
    assert e.value.info["steps_done"] == 1
    assert np.abs(s - j[1]).max() <= 1e-10
    assert err <= BOUNDS["refused"]
    st = up.context(g).stats()
    assert st["transport_nl_steps"] == 1 and st["transport_nl_components"] == 2
    s2, c2, info = up.advance_saturation_components(g, data, s0, c0, 1, acc, ff, c_bc_values=cbv, sorption=ads)
    assert s2.tobytes() == s.tobytes() and c2.tobytes() == c.tobytes() and info["steps_done"] == 1


def errors(lib):
    g = tets(3)
    nc, nf = g.num_cells, g.num_faces
    q = pa.Upwind(KW).darcy_flux(g, VEL)
    bv, acc, s0, ff = inflow_values(g), cfl_accumulation(g, q, 5.0), np.full(nc, 0.1), corey()
    cbv, c0, ads, csrc = tets_components(g, acc, 2)
    up = pa.Upwind(KW, library=lib)
    data = UP.data_for(q, None, bv)
    with pytest.raises(ValueError, match="pfv_upwind_discretize first"):  # a call before discretize
        up.advance_saturation_components(g, data, s0, c0, 1, acc, ff, c_bc_values=cbv)
    up.discretize(g, data)
    ctx = up.context(g)
    dp, ptr = pa._lib._dp, pa._lib._ptr
    for k in (0, 65):  # at both levels
        with pytest.raises(ValueError, match=rf"\({k}, {nc}\)"):
            up.advance_saturation_components(g, data, s0, np.zeros((k, nc)), 1, acc, ff)
        kk = max(k, 1)
        par, s, c, done = np.asarray(ff.params, dtype=float), s0.copy(), np.zeros(kk * nc), C.c_int32(7)
        st = ctx.lib.pfv_transport_advance_nl_multi(ctx._h, None, ff.kind, ptr(par, dp), par.size, ptr(bv, dp), ptr(acc, dp),
                                                    None, None, k, ptr(np.zeros(kk * nf), dp), None, None, 1, 1e-12, 10,
                                                    ptr(s, dp), ptr(c, dp), C.byref(done), None)
        assert st == 4 and done.value == 0
    # wrong shapes, named
    call = lambda **kw: up.advance_saturation_components(g, data, s0, kw.pop("c0", c0), 1, acc, ff, **kw)  # noqa: E731
    with pytest.raises(ValueError, match=rf"c0 .*\({nc},\)"):
        call(c0=c0[0])
    with pytest.raises(ValueError, match=rf"c_bc_values .*\(2, {nf - 1}\)"):
        call(c_bc_values=cbv[:, :-1])
    with pytest.raises(ValueError, match=rf"sorption .*\(3, {nc}\)"):
        call(c_bc_values=cbv, sorption=np.zeros((3, nc)))
    with pytest.raises(ValueError, match=rf"c_source .*\({nc + 1},\)"):
        call(c_bc_values=cbv, c_source=np.zeros(nc + 1))
    with pytest.raises(ValueError, match="s0 must have one entry per cell"):
        up.advance_saturation_components(g, data, s0[:-1], c0, 1, acc, ff)
    with pytest.raises(ValueError, match="flux_function"):
        up.advance_saturation_components(g, data, s0, c0, 1, acc, "corey")
    # the arrays: the lowest cell (face), then its lowest component
    bad = ads.copy()
    bad[1, 5], bad[0, 9] = -1e-3, -1.0
    with pytest.raises(ValueError, match=r"sorption must not be negative: cell 5, component 1$"):
        call(c_bc_values=cbv, sorption=bad)
    bad = ads.copy()
    bad[0, 7] = np.nan
    with pytest.raises(ValueError, match=r"sorption must not be negative: cell 7, component 0$"):
        call(c_bc_values=cbv, sorption=bad)
    for v in (np.nan, np.inf):
        bad = c0.copy()
        bad[:, 11] = v
        bad[0, 40] = v
        with pytest.raises(ValueError, match=r"c is not finite in cell 11, component 0$"):
            call(c0=bad, c_bc_values=cbv)
    cfd = sps.csc_matrix(g.cell_faces)
    bf = g.get_all_boundary_faces()
    inflow = np.array([f for f in bf if (q[f] >= 0) != (sps.find(cfd[f])[2][0] > 0)])
    outflow = np.setdiff1d(bf, inflow)
    bad = cbv.copy()
    bad[:, outflow] = np.nan  # values on outflow faces are not read ...
    bad[:, np.setdiff1d(np.arange(nf), bf)] = np.inf  # ... nor those on interior faces
    s, c, info = call(c_bc_values=bad, sorption=ads, c_source=csrc)
    want = call(c_bc_values=cbv, sorption=ads, c_source=csrc)
    assert info["steps_done"] == 1 and s.tobytes() == want[0].tobytes() and c.tobytes() == want[1].tobytes()
    bad[1, inflow[[2, 4]]] = np.nan
    with pytest.raises(ValueError, match=rf"c_bc_values is not finite on face {inflow[[2, 4]].min()}, component 1$"):
        call(c_bc_values=bad)
    # what the saturation step refuses is refused here in the same words
    a = acc.copy()
    a[5] = 0.0
    with pytest.raises(ValueError, match="accumulation must be positive: cell 5"):
        up.advance_saturation_components(g, data, s0, c0, 1, a, ff, c_bc_values=cbv)
    # a component that is absent everywhere is valid (0 <= 0)
    s, c, info = call(c0=np.vstack([c0[0], np.zeros(nc)]), c_bc_values=np.vstack([cbv[0], np.zeros(nf)]))
    assert info["steps_done"] == 1 and info["c_converged"] == [True, True] and np.all(c[1] == 0.0)


# ---- 9. the handle -----------------------------------------------------------------------------------------------------------
def handle(lib, k=3):
    g, q, ff, bv, acc, s0, _ = _tets_problem(4, "corey")
    cbv, c0, ads, csrc = tets_components(g, acc, k)
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)
    up, data = discretized(lib, g, q, bv, bc)
    ctx = up.context(g)
    run = lambda u, d, n=2: u.advance_saturation_components(g, d, s0, c0, n, acc, ff, c_bc_values=cbv, sorption=ads,  # noqa: E731
                                                            c_source=csrc)
    # no assembly is needed, and none is left behind
    s, c, info = run(up, data)
    assert info["steps_done"] == 2 and ctx.stats()["sweep_order_ms"] > 0
    assert ctx.stats()["transport_nl_components"] == k
    assert ctx.active_size() == 0
    with pytest.raises(RuntimeError):
        ctx.solve()
    with pytest.raises(pa.PorefvError):
        ctx.transport_advance(np.zeros(g.num_cells), 1)
    # the same flux again: the order is kept
    first = ctx.sweep_info()
    s2, c2, _ = run(up, data)
    assert ctx.stats()["sweep_order_ms"] == 0
    assert np.array_equal(first["level"], ctx.sweep_info()["level"])
    assert s2.tobytes() == s.tobytes() and c2.tobytes() == c.tobytes()
    # the plain saturation step on this handle: no components in the statistics
    up.advance_saturation(g, data, s0, 1, acc, ff)
    assert ctx.stats()["transport_nl_components"] == 0 and ctx.stats()["sweep_order_ms"] == 0
    # a selected preconditioner stays selected: the C call below selects nothing itself
    jac, jdata = discretized(lib, g, q, bv, bc)
    c1, i1 = jac.advance(g, jdata, s0, 1, acc, method="gmres")  # selects "jacobi"
    run(jac, jdata, 1)
    jctx = jac.context(g)
    jac._assemble(g, jdata, acc, None, None)
    x, done, last = s0.copy(), C.c_int32(0), pa._lib.SolveInfo()
    st = jctx.lib.pfv_transport_advance(jctx._h, 1, pa._lib.SOLVE_GMRES, 1e-12, 20000, pa._lib._ptr(x, pa._lib._dp),
                                        C.byref(done), C.byref(last))
    assert st == 0 and done.value == 1 and last.iterations == i1["iterations"] > 1
    assert x.tobytes() == c1.tobytes() and jctx.stats()["sweep_direct_steps"] == 0


def flow_system_is_untouched(lib, n=3, k=2):
    """Upwind(flow=mpfa) shares the handle: after the call the flow system assembles and solves to the bits of a handle
    that never saw it (the model: _saturation_cases.flow_system_is_untouched)."""
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
            s, c, info = up.advance_saturation_components(g, tdata, np.full(g.num_cells, 0.1), np.ones((k, g.num_cells)),
                                                          2, acc, corey(), c_bc_values=np.full(g.num_faces, 2.0), maxit=2000)
            assert info["steps_done"] == 2 and s.max() > 0.1 + 1e-6 and c.max() > 1.0 + 1e-6
            assert up.context(g).stats()["transport_nl_components"] == k
        A, b = mp.assemble_matrix_rhs(g, fdata)
        x, info = mp.solve(g, fdata, rtol=1e-12)
        return p, A, b, x, info["iterations"], mp.context(g).matrix(pa._lib.MAT_FLUX)

    p1, A1, b1, x1, it1, F1 = flow(True)
    p2, A2, b2, x2, it2, F2 = flow(False)
    UP.same_csr(A1, A2, "A")
    UP.same_csr(F1, F2, "flux")
    assert p1.tobytes() == p2.tobytes() and np.asarray(b1).tobytes() == np.asarray(b2).tobytes()
    assert x1.tobytes() == x2.tobytes() and it1 == it2

