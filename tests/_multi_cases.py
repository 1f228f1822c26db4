"""Cases of the multi-component transport step (pfv_transport_advance_multi, ``Upwind.advance_components``), shared by
the emulation suite (test_multi_emulation.py) and the GPU suite (test_gpu_multi.py): each takes the library to run on.

Judges: scipy's spsolve on ``diag(acc_a) + A`` with ``A`` and ``b_ref`` as ``assemble_matrix_rhs`` exports them,
component by component; the closed-form recursion of the 1-D line; ``flow_order`` of _sweep_cases for the graph facts."""
import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla

import porepy_amd as pa
from tests import _sweep_cases as SW
from tests import _upwind_cases as UP
from tests._sweep_cases import _injection, cyclic_field, edges, env, flow_order
from tests._upwind_cases import KW, data_for, line_grid, tets


def components(g, k, seed=5):
    """k quantities on the flux of _injection: retardation R_a = 1 + a / 2 on phi V / dt, an own Dirichlet inflow value
    and a random initial state each; the last one is driven by a single source cell from rest (no inflow value, zero
    state: the BiCGStab-breakdown set-up)."""
    q, bc, _, acc0, src = _injection(g)
    rng = np.random.default_rng(seed)
    bf = g.get_all_boundary_faces()
    acc = np.array([(1.0 + 0.5 * a) * acc0 for a in range(k)])
    bv = np.zeros((k, g.num_faces))
    c0 = rng.random((k, g.num_cells))
    source = np.zeros((k, g.num_cells))
    for a in range(k - 1):
        bv[a, bf] = 0.5 * (a + 1)
    c0[k - 1] = 0.0
    source[k - 1] = src
    return q, bc, acc, bv, c0, source


def judge(up, g, q, bc, acc, bv, c0, source, n_steps):
    """spsolve, component by component, on what assemble_matrix_rhs exports; also returns the systems."""
    ref, systems = [], []
    for a in range(c0.shape[0]):
        A, bref = up.assemble_matrix_rhs(g, data_for(q, bc, bv[a]))
        M = (sps.diags(acc[a]) + sps.csr_matrix(A)).tocsc()
        c = c0[a].copy()
        for _ in range(n_steps):
            c = spla.spsolve(M, acc[a] * c - bref + source[a])
        ref.append(c)
        systems.append((M, bref))
    return np.array(ref), systems


def discretized(lib, g, q, bc, bv0):
    data = data_for(q, bc, bv0)
    up = pa.Upwind(KW, library=lib)
    up.discretize(g, data)
    return up, data


# ---- 1. exact against an independent judge ---------------------------------------------------------------------------
def exact(lib, n, k):
    g = tets(n)
    q, bc, acc, bv, c0, source = components(g, k)
    assert flow_order(g.num_cells, *edges(g, q))["core_cells"] == 0
    up, data = discretized(lib, g, q, bc, bv[0])
    ref, _ = judge(up, g, q, bc, acc, bv, c0, source, 3)
    # what one component reports on this handle and flux
    up.advance(g, data, c0[0], 1, acc[0], source=source[0], precond="sweep", rtol=1e-13)
    single = up.context(g).stats()
    assert single["sweep_direct_steps"] == 1
    c, info = up.advance_components(g, data, c0, 3, acc, bc_values=bv, source=source, precond="sweep", rtol=1e-13)
    st = up.context(g).stats()
    err = [np.abs(c[a] - ref[a]).max() / np.abs(ref[a]).max() for a in range(k)]
    print(f"tets({n}), k = {k}: max-norm relative error per component {['%.1e' % e for e in err]}, "
          f"{st['sweep_levels']} levels, {st['sweep_launches']} launches per sweep")
    assert c.shape == (k, g.num_cells) and info["steps_done"] == 3
    assert info["iterations"] == [1] * k and all(info["converged"])
    assert st["transport_multi_components"] == k and st["transport_multi_direct_steps"] == 3
    assert st["transport_multi_fallback_components"] == 0
    assert st["sweep_levels"] == single["sweep_levels"] and st["sweep_launches"] == single["sweep_launches"] > 0
    assert max(err) <= 1e-12
    assert max(info["rel_residual"]) <= 1e-13


# ---- 2. closed form ----------------------------------------------------------------------------------------------------
def closed_form(lib):
    n, qv, dt, phi, k = 16, 0.7, 0.05, 0.3, 3
    g = line_grid(n, 2.0)
    bc = pa.BoundaryCondition(g, g.get_all_boundary_faces(), ["dir", "dir"])
    bv = np.zeros(g.num_faces)
    bv[0] = 1.0
    acc = np.array([(1.0 + 0.5 * a) * phi * g.cell_volumes / dt for a in range(k)])
    up, data = discretized(lib, g, qv * np.ones(g.num_faces), bc, bv)
    want = np.zeros((k, n))
    for a in range(k):
        nu = qv / acc[a]
        c = np.zeros(n)
        for _ in range(10):
            new = np.empty(n)
            for i in range(n):
                new[i] = (c[i] + nu[i] * (new[i - 1] if i else 1.0)) / (1 + nu[i])
            c = new
        want[a] = c
    got, info = up.advance_components(g, data, np.zeros((k, n)), 10, acc, rtol=1e-13, precond="sweep")  # (bc_values: the keyword's)
    st = up.context(g).stats()
    assert info["steps_done"] == 10 and st["transport_multi_direct_steps"] == 10
    assert st["sweep_levels"] == n
    assert np.abs(got - want).max() <= 1e-12
    assert np.abs(want[0] - want[2]).max() > 1e-3  # (the retardation is there)


# ---- 3. agrees with k single runs ---------------------------------------------------------------------------------------
def agrees_with_single_runs(lib, n=4, k=3):
    g = tets(n)
    q, bc, acc, bv, c0, source = components(g, k)
    up, data = discretized(lib, g, q, bc, bv[0])
    c, info = up.advance_components(g, data, c0, 3, acc, bc_values=bv, source=source, precond="sweep", rtol=1e-13)
    assert info["steps_done"] == 3
    for a in range(k):
        one, i1 = up.advance(g, data_for(q, bc, bv[a]), c0[a], 3, acc[a], source=source[a], precond="sweep", rtol=1e-13)
        assert i1["steps_done"] == 3 and up.context(g).stats()["sweep_direct_steps"] == 3
        err = np.abs(c[a] - one).max() / np.abs(one).max()
        print(f"component {a}: relative max-norm difference to the single run {err:.2e}")
        assert err <= 1e-13


# ---- 4. deterministic, and the two launch forms agree -------------------------------------------------------------------
def deterministic_and_merged(lib, n=6, k=3):
    g = tets(n)
    q, bc, acc, bv, c0, source = components(g, k)
    runs = []
    for environment in ({}, {}, {"PFV_SWEEP_MERGE": 0}):
        with env(**environment):
            up, data = discretized(lib, g, q, bc, bv[0])
            c, info = up.advance_components(g, data, c0, 3, acc, bc_values=bv, source=source, precond="sweep", rtol=1e-13)
            st = up.context(g).stats()
        assert info["steps_done"] == 3 and st["transport_multi_direct_steps"] == 3
        runs.append((c, st["sweep_launches"], st["sweep_levels"]))
    print("launches per sweep (merged, merged, one per level):", [r[1] for r in runs])
    assert runs[1][0].tobytes() == runs[0][0].tobytes()
    assert runs[2][0].tobytes() == runs[0][0].tobytes()
    assert runs[2][1] == runs[2][2] and runs[0][1] < runs[2][1]


# ---- 5. a core, or another preconditioner, takes the per-component path ------------------------------------------------------
def core_takes_the_component_path(lib, n_steps=2):
    g, q = cyclic_field()
    assert flow_order(g.num_cells, *edges(g, q))["core_cells"] == 45
    k = 2
    rng = np.random.default_rng(1)
    bf = g.get_all_boundary_faces()
    bv = np.zeros((k, g.num_faces))
    bv[:, bf] = rng.random((k, bf.size))
    vol = np.asarray(g.cell_volumes, dtype=float)
    acc = np.array([vol * (0.5 + rng.random(g.num_cells)) / 0.05 * (1.0 + 0.5 * a) for a in range(k)])
    c0 = rng.random((k, g.num_cells))
    up, data = discretized(lib, g, q, None, bv[0])
    ref, _ = judge(up, g, q, None, acc, bv, c0, np.zeros_like(c0), n_steps)
    c, info = up.advance_components(g, data, c0, n_steps, acc, bc_values=bv, precond="sweep", method="gmres")
    st = up.context(g).stats()
    assert info["steps_done"] == n_steps and all(info["converged"])
    assert st["transport_multi_direct_steps"] == 0 and st["transport_multi_fallback_components"] == 2 * n_steps
    assert st["sweep_core_cells"] == 45
    for a in range(k):
        assert np.abs(c[a] - ref[a]).max() <= 1e-10 * np.abs(ref[a]).max()


def jacobi_takes_the_component_path(lib, n=3, k=3, n_steps=2):
    g = tets(n)
    q, bc, acc, bv, c0, source = components(g, k)
    up, data = discretized(lib, g, q, bc, bv[0])
    ref, _ = judge(up, g, q, bc, acc, bv, c0, source, n_steps)
    c, info = up.advance_components(g, data, c0, n_steps, acc, bc_values=bv, source=source)  # jacobi, BiCGStab
    st = up.context(g).stats()
    assert info["steps_done"] == n_steps and all(info["converged"])
    assert st["transport_multi_direct_steps"] == 0 and st["transport_multi_fallback_components"] == k * n_steps
    assert st["transport_gmres_retries"] >= 1  # (the component from rest breaks BiCGStab down)
    for a in range(k):
        assert np.abs(c[a] - ref[a]).max() <= 1e-10 * np.abs(ref[a]).max()


# ---- 6. a failed check sends only its components to the fallback ----------------------------------------------------------
def failed_check_falls_back(lib, n=3, k=3):
    """The flux handed to the call contradicts the discretization's sign on a few interior faces: the matrix then has
    entries against the flow order, the sweep drops them and the check fails -- for the components that carry
    something across those faces.  The last component is zero throughout (nothing to get wrong): it stays direct."""
    g = tets(n)
    q, bc, acc, bv, c0, source = components(g, k)
    acc = 4.0 * acc  # (the diagonal stays dominant with the contradicting entries)
    c0[k - 1] = 0.0
    source[k - 1] = 0.0
    up, data = discretized(lib, g, q, bc, bv[0])
    interior = np.setdiff1d(np.arange(g.num_faces), g.get_all_boundary_faces())
    q2 = q.copy()
    flip = interior[np.random.default_rng(9).permutation(interior.size)[:4]]
    q2[flip] = -q2[flip]
    rtol = 1e-11
    c, info = up.advance_components(g, data_for(q2, bc, bv[0]), c0, 1, acc, bc_values=bv, source=source, precond="sweep",
                                    method="gmres", rtol=rtol)
    st = up.context(g).stats()
    print(f"contradicting flux on 4 faces: {st['transport_multi_fallback_components']} of {k} components fell back, "
          f"iterations {info['iterations']}")
    assert info["steps_done"] == 1 and all(info["converged"])
    assert 1 <= st["transport_multi_fallback_components"] <= k - 1 and st["transport_multi_direct_steps"] == 0
    assert info["iterations"][k - 1] == 1 and np.all(c[k - 1] == 0.0)
    # the solver stops at a relative residual of rtol; recomputing it on the host moves it by rounding only: a decade
    for a in range(k):
        A, bref = up.assemble_matrix_rhs(g, data_for(q2, bc, bv[a]))
        b = acc[a] * c0[a] - bref + source[a]
        r = b - (sps.diags(acc[a]) + sps.csr_matrix(A)) @ c[a]
        assert np.linalg.norm(r) <= 10 * rtol * np.linalg.norm(b), (a, np.linalg.norm(r), np.linalg.norm(b))


# ---- 7. errors and lifetime ---------------------------------------------------------------------------------------------
def errors(lib):
    g = tets(3)
    nc, nf = g.num_cells, g.num_faces
    q, bc, acc, bv, c0, source = components(g, 2)
    up = pa.Upwind(KW, library=lib)
    data = data_for(q, bc, bv[0])
    # no discretization
    with pytest.raises((ValueError, pa.PorefvError)):
        up.advance_components(g, data, c0, 1, acc, bc_values=bv, precond="sweep")
    up.discretize(g, data)
    # k = 0, k = 65, at both levels
    for k in (0, 65):
        with pytest.raises(ValueError, match=rf"\({k}, {nc}\)"):
            up.advance_components(g, data, np.zeros((k, nc)), 1, acc[0])
        ctx = up.context(g)
        one = np.zeros(max(k, 1) * nc)
        st = ctx.lib.pfv_transport_advance_multi(ctx._h, None, k, pa._lib._ptr(np.zeros(max(k, 1) * nf), pa._lib._dp),
                                                 pa._lib._ptr(one, pa._lib._dp), None, 1, pa._lib.SOLVE_GMRES, 1e-10, 10,
                                                 pa._lib._ptr(one.copy(), pa._lib._dp), None, None)
        assert st == 4
    # wrong shapes, named
    with pytest.raises(ValueError, match=rf"c0 .*\({nc},\)"):
        up.advance_components(g, data, c0[0], 1, acc)
    with pytest.raises(ValueError, match=rf"accumulation .*\(3, {nc}\)"):
        up.advance_components(g, data, c0, 1, np.ones((3, nc)))
    with pytest.raises(ValueError, match=rf"bc_values .*\(2, {nf - 1}\)"):
        up.advance_components(g, data, c0, 1, acc, bc_values=bv[:, :-1])
    with pytest.raises(ValueError, match=rf"source .*\({nc + 1},\)"):
        up.advance_components(g, data, c0, 1, acc, source=np.ones(nc + 1))
    # two components in the discretization: nothing to share
    up2 = pa.Upwind(KW, library=lib)
    d2 = data_for(q, bc, bv[0], k=2)
    up2.discretize(g, d2)
    with pytest.raises((ValueError, pa.PorefvError)):
        up2.advance_components(g, d2, c0, 1, acc, bc_values=bv)
    # periodic grid
    gp = UP.geo(pa.CartGrid([3, 3], [1.0, 1.0]))
    gp.periodic_face_map = np.vstack([np.flatnonzero(np.isclose(gp.face_centers[0], 0.0)),
                                      np.flatnonzero(np.isclose(gp.face_centers[0], 1.0))])
    with pytest.raises(pa.PorefvError) as e:
        pa.Upwind(KW, library=lib).advance_components(gp, data_for(np.ones(gp.num_faces), None, np.zeros(gp.num_faces)),
                                                      np.zeros((2, 9)), 1, np.ones(9))
    assert e.value.status == 5
    # a zero diagonal in one component: named, for both paths
    g1 = line_grid(6, 1.0)
    q1 = np.where(g1.face_centers[0] < 0.5, 1.0, -1.0)  # (cell 2 has inflow from both sides and no outflow)
    d1 = data_for(q1, None, np.zeros(g1.num_faces))
    up1 = pa.Upwind(KW, library=lib)
    up1.discretize(g1, d1)
    acc1 = np.ones((3, 6))
    acc1[1, 2] = 0.0
    for precond in ("sweep", "jacobi"):
        with pytest.raises(pa.PorefvError) as e:
            up1.advance_components(g1, d1, np.zeros((3, 6)), 2, acc1, precond=precond)
        assert e.value.status == 5 and "row 2, component 1" in e.value.message
    c, info = up1.advance_components(g1, d1, np.ones((3, 6)), 2, np.ones((3, 6)), precond="sweep")  # (and without it: fine)
    assert info["steps_done"] == 2


def lifetime(lib, n=4, k=3):
    g = tets(n)
    q, bc, acc, bv, c0, source = components(g, k)
    up, data = discretized(lib, g, q, bc, bv[0])
    ctx = up.context(g)
    # a system assembled before the call is not left behind for solve, nor is one of the call's own
    up.solve(g, data, accumulation=acc[0], c_old=c0[0], precond="sweep")
    up.advance_components(g, data, c0, 2, acc, bc_values=bv, source=source, precond="sweep")
    assert ctx.active_size() == 0
    with pytest.raises(RuntimeError):
        ctx.solve(precond="sweep")
    with pytest.raises(pa.PorefvError):
        ctx.transport_advance(np.zeros(g.num_cells), 1, precond="sweep")
    first = ctx.sweep_info()  # (the order survives)
    SW.same_order(first, flow_order(g.num_cells, *edges(g, q)))
    # a single advance on this handle: the bits of a fresh handle
    one, _ = up.advance(g, data, c0[0], 3, acc[0], source=source[0], precond="sweep", rtol=1e-13)
    assert ctx.stats()["sweep_order_ms"] == 0  # (and with the order that was there)
    fresh, fdata = discretized(lib, g, q, bc, bv[0])
    want, _ = fresh.advance(g, fdata, c0[0], 3, acc[0], source=source[0], precond="sweep", rtol=1e-13)
    assert one.tobytes() == want.tobytes()
    # the same flux again: the order is kept; other edges: rebuilt
    up.advance_components(g, data, c0, 1, acc, bc_values=bv, source=source, precond="sweep")
    assert ctx.stats()["sweep_order_ms"] == 0
    d2 = data_for(-q, bc, bv[0])
    up.discretize(g, d2)
    c, info = up.advance_components(g, d2, c0, 1, acc, bc_values=bv, source=source, precond="sweep")
    assert ctx.stats()["sweep_order_ms"] > 0 and ctx.stats()["transport_multi_direct_steps"] == 1
    second = ctx.sweep_info()
    SW.same_order(second, flow_order(g.num_cells, *edges(g, -q)))
    assert not np.array_equal(first["level"], second["level"])


def flow_system_is_untouched(lib, n=3, k=2):
    """Upwind(flow=mpfa) shares the handle: after the multi-component call the flow system assembles and solves to the
    bits of a handle that never saw it."""
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
            tbv = np.zeros(g.num_faces)
            tbv[g.get_all_boundary_faces()] = 1.0
            tdata = pa.initialize_data({}, KW, {"bc_values": tbv})
            up.discretize(g, tdata)
            acc = 0.2 * g.cell_volumes / 0.05
            c, info = up.advance_components(g, tdata, np.zeros((k, g.num_cells)), 2, acc, precond="sweep")
            assert info["steps_done"] == 2 and c.max() > 0
            assert up.context(g).stats()["transport_multi_components"] == k
        A, b = mp.assemble_matrix_rhs(g, fdata)
        x, info = mp.solve(g, fdata, rtol=1e-12)
        return p, A, b, x, info["iterations"], mp.context(g).matrix(pa._lib.MAT_FLUX)

    p1, A1, b1, x1, it1, F1 = flow(True)
    p2, A2, b2, x2, it2, F2 = flow(False)
    UP.same_csr(A1, A2, "A")
    UP.same_csr(F1, F2, "flux")
    assert p1.tobytes() == p2.tobytes() and np.asarray(b1).tobytes() == np.asarray(b2).tobytes()
    assert x1.tobytes() == x2.tobytes() and it1 == it2
