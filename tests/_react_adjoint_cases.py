"""Cases of the adjoint of the reactive transport step (pfv_transport_adjoint_react,
``Upwind.adjoint_reactive_components``), shared by the emulation suite (test_react_adjoint_emulation.py) and the GPU suite
(test_gpu_react_adjoint.py): each takes the library to run on.

The judge is numpy and scipy: the (k Nc) block system of ``_react_cases.judge`` -- ``diag(acc_a) + w_a A`` on the
diagonal blocks, ``diag(rho) K_ab`` between them, ``A`` as ``assemble_matrix_rhs`` exports it --, the adjoint recursion
``M^T lambda^n = g^n + acc o lambda^{n+1}`` by a sparse LU of ``M^T`` with one step of refinement, and the seven gradient
formulas with the face quantities taken from the discretization's exported matrices.  The judge's formulas themselves
are checked against a complex-step derivative of the forward recursion (``formulas_against_complex_step``).

Errors are max-norm relative per gradient.  The bounds are the project's: 1e-12 for the direct sweep, 1e-10 for a
cyclic core, 1e-13 on the line."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla

import porepy_amd as pa
from tests import _upwind_cases as UP
from tests._adjoint_cases import exported, objective
from tests._multi_cases import components, discretized
from tests._react_cases import chain_with_partner, network
from tests._saturation_cases import cfl_accumulation, inflow_values
from tests._sweep_cases import cyclic_field, edges, env, flow_order, rotation
from tests._upwind_cases import KW, data_for, line_grid, tets

SHARED = ("c0", "source", "bc_values", "accumulation", "flux")
ALL = SHARED + ("rate_matrix", "rate_weight")


# ---- the judge ---------------------------------------------------------------------------------------------------------
def block_system(up, g, q, bc, acc, bv, K, w, rho):
    """(M, bref): the (k Nc) system, component-major unknowns, and b_ref_a (zero for an immobile component, whose
    boundary values are not read)"""
    k, nc = acc.shape
    A, bref = None, np.zeros((k, nc))
    for a in range(k):
        if w[a] > 0 or A is None:
            Aa, ba = up.assemble_matrix_rhs(g, data_for(q, bc, bv[a] if w[a] > 0 else np.zeros(g.num_faces)))
            A = sps.csr_matrix(Aa)
            if w[a] > 0:
                bref[a] = ba
    R = sps.diags(rho)
    blocks = [[(sps.diags(acc[a]) + w[a] * A + K[a, a] * R) if a == b else K[a, b] * R for b in range(k)] for a in range(k)]
    return sps.bmat(blocks, format="csc"), bref


def refined(M):
    """x = M^-1 b by a sparse LU and one step of refinement: exact to rounding"""
    solve = spla.splu(M.tocsc()).solve

    def apply(b):
        x = solve(b)
        return x + solve(b - M @ x)
    return apply


def forward(M, bref, acc, c0, source, w, n_steps):
    """c^0 .. c^N"""
    k, nc = c0.shape
    solve = refined(M)
    states = np.empty((n_steps + 1, k, nc))
    states[0] = c0
    for n in range(n_steps):
        rhs = acc * states[n] - w[:, None] * bref + source
        states[n + 1] = solve(rhs.ravel()).reshape(k, nc)
    return states


def judge(g, data, q, M, acc, bv, K, w, rho, states, loads, obs):
    """The seven gradients of J = sum_n sum_a <loads[n-1, a], c_a^n[obs]>"""
    div, U, D, Nm = exported(g, data)
    n_steps, k = loads.shape[0], loads.shape[1]
    nc, nf = g.num_cells, g.num_faces
    B = div @ (Nm + D @ sps.diags(q))  # bv -> b_ref
    cf = div.T.tocsr()                 # (cf lambda)_f = lambda[p] - lambda[m]
    solve = refined(M.T)
    lam = np.zeros((n_steps + 2, k, nc))
    grads = {"c0": np.zeros((k, nc)), "source": np.zeros((k, nc)), "bc_values": np.zeros((k, nf)),
             "accumulation": np.zeros((k, nc)), "flux": np.zeros(nf), "rate_matrix": np.zeros((k, k)),
             "rate_weight": np.zeros(nc)}
    for n in range(n_steps, 0, -1):
        gn = np.zeros((k, nc))
        gn[:, obs] = loads[n - 1]
        lam[n] = solve((gn + acc * lam[n + 1]).ravel()).reshape(k, nc)
        grads["source"] += lam[n]
        grads["accumulation"] += lam[n] * (states[n - 1] - states[n])
        grads["rate_matrix"] -= (rho * lam[n]) @ states[n].T
        grads["rate_weight"] -= np.sum(lam[n] * (K @ states[n]), axis=0)
        for a in range(k):
            if w[a] > 0:
                grads["bc_values"][a] -= w[a] * (B.T @ lam[n, a])
                grads["flux"] -= w[a] * (cf @ lam[n, a]) * (U @ states[n, a] + D @ bv[a])
    grads["c0"] = acc * lam[1]
    return grads


def relative_errors(got, ref, names=ALL):
    """max-norm relative error per gradient"""
    return {m: float(np.abs(got[m] - ref[m]).max() / np.abs(ref[m]).max()) for m in names}


def cell_weight(g, seed):
    return np.asarray(g.cell_volumes, dtype=float) / 0.02 * (0.5 + np.random.default_rng(seed).random(g.num_cells))


def one_network(k):
    if k == 1:
        return np.array([[0.7]]), np.ones(1)
    return network(k)


def problem(lib, g, k, n_steps, n_obs=5, seed=11, bc=None, bv=None, K=None, w=None):
    """The k components of _multi_cases on g under the network of k components, a random weight per cell, the judge's
    forward run and random loads on n_obs cells."""
    q, bc0, acc, bv0, c0, source = components(g, k)
    bc = bc0 if bc is None else bc
    bv = bv0 if bv is None else bv
    K0, w0 = one_network(k)
    K = K0 if K is None else K
    w = w0 if w is None else w
    rho = cell_weight(g, seed + 1)
    rng = np.random.default_rng(seed)
    obs = np.sort(rng.permutation(g.num_cells)[:n_obs])
    loads = rng.standard_normal((n_steps, k, n_obs))
    up, data = discretized(lib, g, q, bc, bv[0] if w[0] > 0 else np.zeros(g.num_faces))
    M, bref = block_system(up, g, q, bc, acc, bv, K, w, rho)
    states = forward(M, bref, acc, c0, source, w, n_steps)
    return dict(g=g, q=q, bc=bc, acc=acc, bv=bv, c0=c0, source=source, K=K, w=w, rho=rho, obs=obs, loads=loads, up=up,
                data=data, M=M, states=states, n_steps=n_steps, k=k)


def adjoint(p, want=ALL, **kw):
    args = dict(rate_weight=p["rho"], mobility=p["w"], obs_cells=p["obs"], states=p["states"], bc_values=p["bv"], want=want)
    args.update(kw)
    return p["up"].adjoint_reactive_components(p["g"], p["data"], p["n_steps"], p["acc"], p["K"], p["loads"], **args)


def judged(p):
    return judge(p["g"], p["data"], p["q"], p["M"], p["acc"], p["bv"], p["K"], p["w"], p["rho"], p["states"], p["loads"],
                 p["obs"])


# ---- 1. the judge's formulas against a complex-step derivative -------------------------------------------------------------
def formulas_against_complex_step(lib, n=3, k=4, n_steps=3, picks=20, h=1e-30):
    """J(K + i h e_ab), J(rho + i h e_i), J(q + i h e_f), ... by the forward recursion in complex arithmetic, rebuilt
    from the exported matrices alone: Im J / h is the derivative to rounding (no subtraction).  Bound 1e-9 of the
    gradient's largest entry: this checks algebra, not rounding.  k = 4: the chain with the immobile partner, whose K
    has structural zeros.  20 picks per gradient; K has 16 entries, all of which are taken."""
    g = tets(n)
    q, _, acc, bv, c0, source = components(g, k)
    bf = g.get_all_boundary_faces()
    labels = np.where(g.face_centers[2, bf] < 1e-9, "neu", "dir")  # the bottom: Neumann; the rest: Dirichlet
    bc = pa.BoundaryCondition(g, bf, list(labels))
    rng = np.random.default_rng(3)
    bv = bv.copy()
    bv[:, bf] = rng.random((k, bf.size))
    p = problem(lib, g, k, n_steps, bc=bc, bv=bv)
    K, w, rho = p["K"], p["w"], p["rho"]
    assert (w == 0).any() and (K == 0).any()
    ref = judged(p)
    div, U, D, Nm = exported(g, p["data"])
    obs, loads = p["obs"], p["loads"]
    nc = g.num_cells

    def J(qz, accz, bvz, c0z, srcz, Kz, rhoz):
        A = div @ sps.diags(qz) @ U
        R = sps.diags(rhoz)
        M = sps.bmat([[(sps.diags(accz[a]) + w[a] * A + Kz[a, a] * R) if a == b else Kz[a, b] * R for b in range(k)]
                      for a in range(k)], format="csc")
        solve = spla.splu(M).solve
        bref = np.array([w[a] * (div @ (Nm @ bvz[a] + D @ (qz * bvz[a]))) for a in range(k)])
        c, tot = c0z, 0.0
        for s in range(n_steps):
            c = solve((accz * c - bref + srcz).ravel()).reshape(k, nc)
            tot = tot + np.sum(loads[s] * c[:, obs])
        return tot

    base = [x.astype(complex) for x in (p["q"], acc, bv, c0, source, K, rho)]
    assert abs(J(*base).real - objective(p["states"], loads, obs)) <= 1e-10 * np.abs(loads).sum()
    # faces of every kind: interior, Dirichlet inflow, Dirichlet outflow, Neumann
    is_b = np.zeros(g.num_faces, dtype=bool)
    is_b[bf] = True
    neu = np.zeros(g.num_faces, dtype=bool)
    neu[bf[labels == "neu"]] = True
    dirin = np.asarray(np.abs(D).sum(axis=1)).ravel() > 0
    kinds = {"interior": ~is_b, "dirichlet inflow": dirin, "dirichlet outflow": is_b & ~neu & ~dirin, "neumann": neu}
    faces = np.concatenate([rng.permutation(np.flatnonzero(m))[:picks // 4] for m in kinds.values()])
    assert all(m.any() for m in kinds.values()) and faces.size == picks
    # cells with the smallest and the largest weight among the picks
    by_rho = np.argsort(rho)
    cells = np.concatenate([by_rho[:2], by_rho[-2:], rng.permutation(by_rho[2:-2])[:picks - 4]])
    # every entry of K: diagonal, off-diagonal, structurally zero
    entries = [(a, b) for a in range(k) for b in range(k)]
    assert any(a != b and K[a, b] != 0 for a, b in entries) and any(K[a, b] == 0 for a, b in entries)
    worst = {}
    for name, slot in (("flux", 0), ("accumulation", 1), ("bc_values", 2), ("c0", 3), ("source", 4), ("rate_matrix", 5),
                       ("rate_weight", 6)):
        scale = np.abs(ref[name]).max()
        err = 0.0
        for t in range(len(entries) if name == "rate_matrix" else picks):
            z = [x.copy() for x in base]
            if name == "flux":
                idx = (faces[t],)
            elif name == "bc_values":
                idx = (rng.integers(k), faces[t])
            elif name == "rate_matrix":
                idx = entries[t]
            elif name == "rate_weight":
                idx = (cells[t],)
            else:
                idx = (rng.integers(k), rng.integers(nc))
            z[slot][idx] += 1j * h
            err = max(err, abs(J(*z).imag / h - ref[name][idx]) / scale)
        worst[name] = err
    print("complex step against the judge, relative to the gradient's largest entry:",
          {m: "%.1e" % e for m, e in worst.items()})
    assert np.abs(ref["bc_values"][:, ~(neu | dirin)]).max() == 0.0 and np.abs(ref["flux"][neu]).max() == 0.0
    assert np.abs(ref["bc_values"][w == 0]).max() == 0.0
    assert max(worst.values()) <= 1e-9
    # the library on this problem, the only one with Neumann faces: the judge that was just judged, bound of the sweep
    grads, info = adjoint(p)
    err = relative_errors(grads, ref)
    print("the library against the judge, Neumann bottom:", {m: "%.1e" % e for m, e in err.items()})
    assert info["steps_done"] == n_steps and max(err.values()) <= 1e-12
    assert np.abs(grads["bc_values"][:, neu]).max() > 0 and np.abs(grads["flux"][neu]).max() == 0.0


# ---- 2. the library against the judge --------------------------------------------------------------------------------
def exact(lib, n, k, n_steps=3):
    g = tets(n)
    p = problem(lib, g, k, n_steps)
    assert flow_order(g.num_cells, *edges(g, p["q"]))["core_cells"] == 0
    ref = judged(p)
    up = p["up"]
    up.advance_reactive_components(g, p["data"], p["c0"], 1, p["acc"], p["K"], rate_weight=p["rho"], mobility=p["w"],
                                   bc_values=p["bv"], source=p["source"])
    fwd = up.context(g).stats()
    grads, info = adjoint(p)
    st = up.context(g).stats()
    err = relative_errors(grads, ref)
    print(f"tets({n}), k = {k}: max-norm relative error per gradient", {m: "%.1e" % e for m, e in err.items()},
          f"{st['sweep_levels']} levels, {st['sweep_launches']} launches per transposed sweep")
    assert info["steps_done"] == n_steps and info["converged"] and info["iterations"] == [1] * k
    assert st["sweep_levels"] == fwd["sweep_levels"] and st["sweep_launches"] == fwd["sweep_launches"] > 0
    assert st["transport_react_adjoint_steps"] == n_steps and st["transport_react_adjoint_core_iterations"] == 0
    assert grads["c0"].shape == (k, g.num_cells) and grads["bc_values"].shape == (k, g.num_faces)
    assert grads["flux"].shape == (g.num_faces,) and grads["rate_matrix"].shape == (k, k)
    assert grads["rate_weight"].shape == (g.num_cells,)
    assert max(err.values()) <= 1e-12


# ---- 3. K = 0, w = 1: the uncoupled adjoint ----------------------------------------------------------------------------
def reduces_to_uncoupled(lib, n=4, k=3, n_steps=3):
    g = tets(n)
    p = problem(lib, g, k, n_steps, K=np.zeros((k, k)), w=np.ones(k))
    grads, info = adjoint(p)
    lin, ldata = discretized(lib, g, p["q"], p["bc"], p["bv"][0])
    want, linfo = lin.adjoint_components(g, ldata, n_steps, p["acc"], p["loads"], obs_cells=p["obs"], states=p["states"],
                                         bc_values=p["bv"], want=SHARED)
    assert info["steps_done"] == n_steps and linfo["steps_done"] == n_steps
    for m in SHARED:
        assert grads[m].tobytes() == want[m].tobytes(), m
    # without the optional arguments: mobility None = 1, rate_weight None = 1
    plain, _ = adjoint(p, want=SHARED, rate_weight=None, mobility=None)
    for m in SHARED:
        assert plain[m].tobytes() == want[m].tobytes(), m
    ref = judged(p)
    err = relative_errors(grads, ref, ("rate_matrix",))
    print(f"K = 0: grad_rate against the judge {err['rate_matrix']:.1e}, largest entry {np.abs(ref['rate_matrix']).max():.2e}")
    assert np.abs(ref["rate_matrix"]).max() > 0 and err["rate_matrix"] <= 1e-12
    assert np.abs(grads["rate_weight"]).max() == 0.0  # (K c = 0)


# ---- 4. the immobile partner -------------------------------------------------------------------------------------------
def immobile_partner(lib, n=3, n_steps=3):
    g = tets(n)
    q, bc, acc, bv, c0, source = components(g, 4)
    bv[3] = np.nan
    p = problem(lib, g, 4, n_steps, bv=bv)
    assert p["w"][3] == 0.0
    grads, info = adjoint(p)
    ref = judged(p)
    assert info["steps_done"] == n_steps
    for m in ALL:
        assert np.isfinite(grads[m]).all(), m
    assert np.abs(grads["bc_values"][3]).max() == 0.0
    err = relative_errors(grads, ref)
    print("immobile partner with NaN boundary values:", {m: "%.1e" % e for m, e in err.items()})
    assert err["flux"] <= 1e-12 and max(err.values()) <= 1e-12
    # the same NaN under a mobile component is refused, with its face and component
    w2 = p["w"].copy()
    w2[3] = 0.5
    with pytest.raises(ValueError, match=r"bc_values is not finite on face \d+, component 3$"):
        adjoint(p, mobility=w2)


# ---- 5. the adjoint identity with the library's own forward ----------------------------------------------------------
def identity_with_own_forward(lib, n=4, k=4, n_steps=4):
    """J is linear and homogeneous in (c0, source, bc_values): J = <grad_c0, c0> + <grad_source, src> + <grad_bc, bv>."""
    g = tets(n)
    p = problem(lib, g, k, n_steps)
    up = p["up"]
    states = np.empty_like(p["states"])
    states[0] = p["c0"]
    for s in range(n_steps):
        states[s + 1], info = up.advance_reactive_components(g, p["data"], states[s], 1, p["acc"], p["K"],
                                                             rate_weight=p["rho"], mobility=p["w"], bc_values=p["bv"],
                                                             source=p["source"])
        assert info["steps_done"] == 1
    grads, info = adjoint(p, want=("c0", "source", "bc_values"), states=None)
    assert info["steps_done"] == n_steps and sorted(grads) == ["bc_values", "c0", "source"]
    terms = [np.sum(grads["c0"] * p["c0"]), np.sum(grads["source"] * p["source"]), np.sum(grads["bc_values"] * p["bv"])]
    J = objective(states, p["loads"], p["obs"])
    print(f"J = {J:.15e}, the three products {terms}, difference {J - sum(terms):.2e}")
    assert abs(J - sum(terms)) <= 1e-11 * np.abs(terms).sum()


# ---- 6. the line's closed form -----------------------------------------------------------------------------------------
def line_closed_form(lib, n=16, n_steps=3):
    """16 cells, the chain of three of _react_cases.closed_form: forward and backward cell by cell with
    numpy.linalg.solve.  Row i of the transposed system: B_i^T lam_i - q lam_{i+1} = r_i."""
    qv, dt, phi, k = 0.7, 0.05, 0.3, 3
    g = line_grid(n, 2.0)
    bc = pa.BoundaryCondition(g, g.get_all_boundary_faces(), ["dir", "dir"])
    bv = np.zeros((k, g.num_faces))
    bv[0, 0] = 1.0
    acc = np.array([(1.0 + 0.5 * a) * phi * g.cell_volumes / dt for a in range(k)])
    K = np.array([[2.0, 0.0, 0.0], [-2.0, 1.0, 0.0], [0.0, -1.0, 0.25]])
    rho = phi * np.asarray(g.cell_volumes, dtype=float) * (1.0 + 0.1 * np.arange(n))
    up, data = discretized(lib, g, qv * np.ones(g.num_faces), bc, bv[0])
    blocks = [np.diag(acc[:, i] + qv) + rho[i] * K for i in range(n)]
    states = np.zeros((n_steps + 1, k, n))
    for s in range(n_steps):
        for i in range(n):
            inflow = states[s + 1][:, i - 1] if i else bv[:, 0]
            states[s + 1][:, i] = np.linalg.solve(blocks[i], acc[:, i] * states[s][:, i] + qv * inflow)
    loads = np.zeros((n_steps, k, 1))
    loads[n_steps - 1, 2, 0] = 1.0  # the granddaughter at the outlet, at the last step
    lam = np.zeros((n_steps + 2, k, n))
    for s in range(n_steps, 0, -1):
        rhs = acc * lam[s + 1]
        rhs[:, n - 1] += loads[s - 1, :, 0]
        for i in range(n - 1, -1, -1):
            lam[s][:, i] = np.linalg.solve(blocks[i].T, rhs[:, i] + (qv * lam[s][:, i + 1] if i + 1 < n else 0.0))
    want = {"source": lam[1:n_steps + 1].sum(axis=0), "c0": acc * lam[1],
            "rate_matrix": -sum((rho * lam[s]) @ states[s].T for s in range(1, n_steps + 1)),
            "rate_weight": -sum(np.sum(lam[s] * (K @ states[s]), axis=0) for s in range(1, n_steps + 1))}
    grads, info = up.adjoint_reactive_components(g, data, n_steps, acc, K, loads, rate_weight=rho, obs_cells=[n - 1],
                                                 states=states, bc_values=bv, want=tuple(want))
    st = up.context(g).stats()
    assert info["steps_done"] == n_steps and st["sweep_levels"] == n
    err = relative_errors(grads, want, tuple(want))
    print("line, chain of three:", {m: "%.1e" % e for m, e in err.items()})
    assert max(err.values()) <= 1e-13
    assert want["c0"][0, 0] > 0  # (the load on the granddaughter at the outlet reaches the parent in the inlet cell)


# ---- 7. launch forms and determinism ------------------------------------------------------------------------------------
def launch_forms_and_determinism(lib, n=6, k=4, n_steps=2):
    g = tets(n)
    runs = []
    p = None
    for environment in ({}, {}, {"PFV_SWEEP_MERGE": 0}, {"PFV_SWEEP_MERGE_ROWS": 24}):
        with env(**environment):
            if p is None:
                p = problem(lib, g, k, n_steps)
            else:
                p["up"], p["data"] = discretized(lib, g, p["q"], p["bc"], p["bv"][0])
            grads, info = adjoint(p)
            st = p["up"].context(g).stats()
        assert info["steps_done"] == n_steps
        runs.append((grads, st["sweep_launches"], st["sweep_levels"]))
    print("launches per transposed sweep (merged, merged, one per level, runs of <= 24 rows):", [r[1] for r in runs])
    for r in runs[1:]:
        for m in ALL:
            assert r[0][m].tobytes() == runs[0][0][m].tobytes(), m
    assert runs[2][1] == runs[2][2] and runs[0][1] < runs[3][1] < runs[2][1]
    again, _ = adjoint(p)  # a repeat on the same handle
    for m in ALL:
        assert again[m].tobytes() == runs[0][0][m].tobytes(), m
    assert max(relative_errors(again, judged(p)).values()) <= 1e-12


# ---- 8. a cyclic core ----------------------------------------------------------------------------------------------------
def cyclic_core(lib, name, k=4, n_steps=2):
    g, q = cyclic_field(12) if name == "cyclic12" else rotation(8)
    core_cells = flow_order(g.num_cells, *edges(g, q))["core_cells"]
    assert core_cells == {"cyclic12": 45, "rotation8": 64}[name]
    nc = g.num_cells
    K, w = chain_with_partner()
    rng = np.random.default_rng(5)
    acc0 = cfl_accumulation(g, q, 2.0)
    acc = np.array([(1.0 + 0.5 * a) * acc0 for a in range(k)])
    rho = acc0 * (0.5 + rng.random(nc))
    bv = np.array([(0.5 + 0.25 * a) * inflow_values(g, 1.0) for a in range(k)])
    c0 = 0.2 + rng.random((k, nc))
    source = np.zeros((k, nc))
    obs = np.sort(rng.permutation(nc)[:5])
    loads = rng.standard_normal((n_steps, k, 5))
    up, data = discretized(lib, g, q, None, bv[0])
    M, bref = block_system(up, g, q, None, acc, bv, K, w, rho)
    states = forward(M, bref, acc, c0, source, w, n_steps)
    ref = judge(g, data, q, M, acc, bv, K, w, rho, states, loads, obs)
    args = dict(rate_weight=rho, mobility=w, obs_cells=obs, states=states, bc_values=bv, want=ALL)
    grads, info = up.adjoint_reactive_components(g, data, n_steps, acc, K, loads, **args)
    st = up.context(g).stats()
    err = relative_errors(grads, ref)
    print(f"{name}: {core_cells} core cells, {st['transport_react_adjoint_core_iterations']} core iterations in all, "
          "max-norm relative error per gradient", {m: "%.1e" % e for m, e in err.items()})
    assert info["steps_done"] == n_steps and info["converged"]
    assert st["sweep_core_cells"] == core_cells and st["transport_react_adjoint_core_iterations"] > 0
    assert info["iterations"][0] > 1 and info["iterations"] == [info["iterations"][0]] * k
    assert max(err.values()) <= 1e-10
    # one iteration is not enough: the step is refused, no gradient is written
    none, info = up.adjoint_reactive_components(g, data, n_steps, acc, K, loads, maxit=1, raise_on_fail=False, **args)
    assert info["steps_done"] == 0 and not info["converged"]
    for m in ALL:
        assert not none[m].any(), m
    with pytest.raises(pa.PorefvError) as e:
        up.adjoint_reactive_components(g, data, n_steps, acc, K, loads, maxit=1, **args)
    assert e.value.status == 6 and "did not settle" in e.value.message


# ---- 9. the two forms of the observation ----------------------------------------------------------------------------------
def observation_forms(lib, n=3, k=4, n_steps=3):
    p = problem(lib, tets(n), k, n_steps)
    p["loads"][0, 1, 0] = 0.0  # (a zero among the loads of an observed cell, as on every cell that is not observed)
    sparse, _ = adjoint(p)
    dense_loads = np.zeros((n_steps, k, p["g"].num_cells))
    dense_loads[:, :, p["obs"]] = p["loads"]
    dense, info = p["up"].adjoint_reactive_components(
        p["g"], p["data"], n_steps, p["acc"], p["K"], dense_loads, rate_weight=p["rho"], mobility=p["w"], obs_cells=None,
        states=p["states"], bc_values=p["bv"], want=ALL)
    assert info["steps_done"] == n_steps
    for m in ALL:
        assert dense[m].tobytes() == sparse[m].tobytes(), m
    # the order of the observation cells does not matter either
    perm = np.random.default_rng(2).permutation(p["obs"].size)
    shuffled, _ = p["up"].adjoint_reactive_components(
        p["g"], p["data"], n_steps, p["acc"], p["K"], p["loads"][:, :, perm], rate_weight=p["rho"], mobility=p["w"],
        obs_cells=p["obs"][perm], states=p["states"], bc_values=p["bv"], want=ALL)
    for m in ALL:
        assert shuffled[m].tobytes() == sparse[m].tobytes(), m


# ---- 10. refusals ---------------------------------------------------------------------------------------------------------
def _c_call(ctx, p, k=None, states=True, which=None, n_steps=None):
    """pfv_transport_adjoint_react with host arrays; `which`: positions of the gradients asked for (15 .. 21)"""
    dp, ip, ptr = pa._lib._dp, pa._lib._ip, pa._lib._ptr
    k = p["k"] if k is None else k
    g = p["g"]
    nc, nf = g.num_cells, g.num_faces
    m = max(k, 1)
    keep = [np.ascontiguousarray(x) for x in (p["bv"], p["acc"], p["w"], p["K"], p["rho"], p["loads"], p["states"])]
    if k != p["k"]:
        keep[:4] = [np.zeros(m * nf), np.ones(m * nc), np.ones(m), np.zeros(m * m)]
    obs32 = p["obs"].astype(np.int32)
    out = np.zeros(max(m * nc, m * nf, m * m))
    args = [ctx._h, None, k, ptr(keep[0], dp), ptr(keep[1], dp), ptr(keep[2], dp), ptr(keep[3], dp), ptr(keep[4], dp),
            p["n_steps"] if n_steps is None else n_steps, obs32.size, ptr(obs32, ip), ptr(keep[5], dp),
            ptr(keep[6], dp) if states else None, 1e-12, 10, None, None, None, None, None, None, None, None, None]
    for pos in which or ():
        args[pos] = ptr(out, dp)
    st = ctx.lib.pfv_transport_adjoint_react(*args)
    return st, ctx.lib.pfv_last_error(ctx._h).decode()


def refusals(lib, n=3, k=4, n_steps=2):
    g = tets(n)
    nc = g.num_cells
    p = problem(lib, g, k, n_steps)
    up, data, acc, K, loads, obs = p["up"], p["data"], p["acc"], p["K"], p["loads"], p["obs"]
    w, rho = p["w"], p["rho"]
    # no discretization on the handle, at both levels
    bare = pa.Upwind(KW, library=lib)
    with pytest.raises(ValueError, match="pfv_upwind_discretize first"):
        bare.adjoint_reactive_components(g, data, n_steps, acc, K, loads, rate_weight=rho, mobility=w, obs_cells=obs,
                                         bc_values=p["bv"])
    st, text = _c_call(bare.context(g), p)
    assert st == 4 and text == "pfv_upwind_discretize first", text

    def refused(match, **change):
        a = dict(acc=acc, K=K, loads=loads, rate_weight=rho, mobility=w, obs_cells=obs, bc_values=p["bv"])
        a.update(change)
        acc_, K_, loads_ = a.pop("acc"), a.pop("K"), a.pop("loads")
        with pytest.raises(ValueError, match=match):
            up.adjoint_reactive_components(g, data, n_steps, acc_, K_, loads_, **a)

    def changed(x, idx, v):
        y = np.array(x, dtype=float, copy=True)
        y[idx] = v
        return y

    # an inadmissible or non-finite K, in the caller's orientation (rate[a][b], not its transpose)
    refused(r"rate\[2\]\[2\] is negative", K=changed(K, (2, 2), -0.1))
    refused(r"rate\[1\]\[3\] is positive", K=changed(K, (1, 3), 0.1))
    refused(r"column 1 of rate has a negative sum", K=changed(K, (2, 1), -0.5 - 1e-9))
    refused(r"rate\[0\]\[3\] is not finite", K=changed(K, (0, 3), np.nan))
    refused(r"mobility\[1\] is negative", mobility=changed(w, 1, -1.0))
    refused(r"rate_weight must not be negative: cell 7$", rate_weight=changed(changed(rho, 7, -1.0), 30, -1.0))
    refused(r"accumulation must be positive: cell 11, component 2$", acc=changed(changed(acc, (2, 11), 0.0), (0, 40), 0.0))
    # observation cells and loads
    bad = obs.copy()
    bad[2] = obs[0]
    refused(rf"obs_cells\[2\] = {obs[0]} is repeated", obs_cells=bad)
    bad[2] = nc
    refused(rf"obs_cells\[2\] = {nc} is out of range", obs_cells=bad)
    for value in (np.nan, np.inf):
        refused("loads is not finite at step 2, component 1, observation 3", loads=changed(loads, (1, 1, 3), value))
    # the gradients that need the states, at both levels
    for name in ("accumulation", "flux", "rate_matrix", "rate_weight"):
        refused(rf'"{name}" needs states', want=("c0", name))
    refused("unknown gradient 'mobility'", want=("mobility",))
    ctx = up.context(g)
    for pos, name in ((18, "grad_accumulation"), (19, "grad_flux"), (20, "grad_rate"), (21, "grad_rate_weight")):
        st, text = _c_call(ctx, p, states=False, which=(pos,))
        assert st == 4 and text.startswith(name + " needs states"), (name, text)
    # k = 0 and k = 9, at both levels
    for kk in (0, 9):
        st, text = _c_call(ctx, p, k=kk, n_steps=0)
        assert st == 4 and f"k = {kk}" in text
        with pytest.raises(ValueError, match=rf"1 \.\. 8, not {kk} "):
            up.adjoint_reactive_components(g, data, n_steps, acc[0], np.zeros((kk, kk)), np.zeros((n_steps, kk, obs.size)),
                                           obs_cells=obs)
    # shapes, named
    refused(r"rate_matrix must have shape \(4, 4\), not \(3, 3\)", K=np.zeros((3, 3)))
    refused(r"mobility must have shape \(4,\)", mobility=np.ones(3))
    refused(rf"loads .*\({n_steps}, {k}, {obs.size}\)", loads=loads[:, :, :-1])
    refused(rf"states .*\({n_steps + 1}, {k}, {nc}\)", states=p["states"][1:], want=ALL)
    # two components in the discretization: nothing to share
    up2 = pa.Upwind(KW, library=lib)
    d2 = data_for(p["q"], p["bc"], p["bv"][0], k=2)
    up2.discretize(g, d2)
    with pytest.raises((ValueError, pa.PorefvError), match="num_components = 1"):
        up2.adjoint_reactive_components(g, d2, n_steps, acc, K, loads, obs_cells=obs)
    # after all the refusals the handle still computes the gradients
    grads, info = adjoint(p)
    assert info["steps_done"] == n_steps
    assert max(relative_errors(grads, judged(p)).values()) <= 1e-12


# ---- 11. the handle ------------------------------------------------------------------------------------------------------
def handle(lib, n=4, k=4, n_steps=2):
    g = tets(n)
    p = problem(lib, g, k, n_steps)
    up, data, q, bc = p["up"], p["data"], p["q"], p["bc"]
    ctx = up.context(g)
    forward_args = dict(rate_weight=p["rho"], mobility=p["w"], bc_values=p["bv"], source=p["source"])
    before, _ = up.advance_reactive_components(g, data, p["c0"], 2, p["acc"], p["K"], **forward_args)
    up.solve(g, data, accumulation=p["acc"][0], c_old=p["c0"][0], precond="sweep")  # (an assembled system on the handle)
    first, _ = adjoint(p)
    # no transport system is left behind; the order is
    assert ctx.active_size() == 0
    with pytest.raises(RuntimeError):
        ctx.solve(precond="sweep")
    after, _ = up.advance_reactive_components(g, data, p["c0"], 2, p["acc"], p["K"], **forward_args)
    assert ctx.stats()["sweep_order_ms"] == 0  # (with the order that was there)
    assert after.tobytes() == before.tobytes()
    # the same flux again: the order and the transposed positions are kept, also across the uncoupled adjoint
    again, _ = adjoint(p)
    assert ctx.stats()["sweep_order_ms"] == 0
    up.adjoint_components(g, data, n_steps, p["acc"], p["loads"], obs_cells=p["obs"], bc_values=np.nan_to_num(p["bv"]))
    third, _ = adjoint(p)
    for m in ALL:
        assert again[m].tobytes() == first[m].tobytes() and third[m].tobytes() == first[m].tobytes(), m
    # a fresh handle builds the order and the positions by itself
    fresh, fdata = discretized(lib, g, q, bc, p["bv"][0])
    g2, _ = adjoint(dict(p, up=fresh, data=fdata))
    assert fresh.context(g).stats()["sweep_order_ms"] > 0
    for m in ALL:
        assert g2[m].tobytes() == first[m].tobytes(), m
    # a discretization with other edges: the pattern's positions are dropped with it, the gradients are the new flux's
    d2 = data_for(-q, bc, p["bv"][0])
    up.discretize(g, d2)
    M2, bref2 = block_system(up, g, -q, bc, p["acc"], p["bv"], p["K"], p["w"], p["rho"])
    states2 = forward(M2, bref2, p["acc"], p["c0"], p["source"], p["w"], n_steps)
    p2 = dict(p, q=-q, data=d2, M=M2, states=states2)
    got2, info = adjoint(p2)
    assert info["steps_done"] == n_steps and ctx.stats()["sweep_order_ms"] > 0
    assert max(relative_errors(got2, judged(p2)).values()) <= 1e-12


def flow_system_is_untouched(lib, n=3, k=4):
    """Upwind(flow=mpfa) shares the handle: after the adjoint call the flow system assembles and solves to the bits of
    a handle that never saw it, with the preconditioner that was selected."""
    K, w = chain_with_partner()

    def flow(with_adjoint):
        g = tets(n)
        fdata, _ = UP.flow_problem(g, np.random.default_rng(23))
        mp = pa.Mpfa("flow", library=lib)
        mp.discretize(g, fdata)
        pr, _ = mp.solve(g, fdata, rtol=1e-12)
        if with_adjoint:
            mp.darcy_flux(g, fdata, pr, resident=True)
            up = pa.Upwind(KW, library=lib, flow=mp)
            assert up.context(g) is mp.context(g)
            tbv = np.zeros(g.num_faces)
            tbv[g.get_all_boundary_faces()] = 1.0
            tdata = pa.initialize_data({}, KW, {"bc_values": tbv})
            up.discretize(g, tdata)
            acc = 0.2 * g.cell_volumes / 0.05
            grads, info = up.adjoint_reactive_components(g, tdata, 2, acc, K, np.ones((2, k, g.num_cells)), mobility=w)
            assert info["steps_done"] == 2 and np.abs(grads["c0"]).max() > 0
            assert up.context(g).stats()["transport_react_adjoint_steps"] == 2
        A, b = mp.assemble_matrix_rhs(g, fdata)
        x, info = mp.solve(g, fdata, rtol=1e-12)
        return pr, A, b, x, info["iterations"], mp.context(g).matrix(pa._lib.MAT_FLUX)

    p1, A1, b1, x1, it1, F1 = flow(True)
    p2, A2, b2, x2, it2, F2 = flow(False)
    UP.same_csr(A1, A2, "A")
    UP.same_csr(F1, F2, "flux")
    assert p1.tobytes() == p2.tobytes() and np.asarray(b1).tobytes() == np.asarray(b2).tobytes()
    assert x1.tobytes() == x2.tobytes() and it1 == it2


# ---- 12. device-resident vectors ---------------------------------------------------------------------------------------
def device_vectors(lib, to_device=None, to_host=None, n=3, k=4, n_steps=2):
    """Every vector of the call in device memory (pfv_set_vectors_on_device; obs_cells, rate, mobility and grad_rate
    stay on the host): the bits of the host-array call.  ``to_device(array) -> (address, keepalive)``,
    ``to_host(keepalive) -> array``; the emulation build takes host addresses."""
    if to_device is None:
        to_device = lambda a: (a.ctypes.data, a)  # noqa: E731
        to_host = lambda a: a  # noqa: E731
    p = problem(lib, tets(n), k, n_steps)
    want, _ = adjoint(p)
    g, ctx = p["g"], p["up"].context(p["g"])
    nc, nf = g.num_cells, g.num_faces
    dp = pa._lib._dp

    def dev(a):
        addr, keep = to_device(np.ascontiguousarray(a, dtype=np.float64))
        return C.cast(addr, dp), keep

    ins = [dev(x) for x in (p["q"], p["bv"], p["acc"], p["rho"], p["loads"], p["states"])]
    outs = {name: dev(np.zeros(m)) for name, m in (("c0", k * nc), ("source", k * nc), ("bc_values", k * nf),
                                                   ("accumulation", k * nc), ("flux", nf), ("rate_weight", nc))}
    gK = np.zeros((k, k))
    Kc, wc = np.ascontiguousarray(p["K"]), np.ascontiguousarray(p["w"])
    obs32 = p["obs"].astype(np.int32)
    done = C.c_int32(0)
    ctx._dev(True)
    try:
        st = ctx.lib.pfv_transport_adjoint_react(
            ctx._h, ins[0][0], k, ins[1][0], ins[2][0], pa._lib._ptr(wc, dp), pa._lib._ptr(Kc, dp), ins[3][0], n_steps,
            obs32.size, pa._lib._ptr(obs32, pa._lib._ip), ins[4][0], ins[5][0], 1e-12, 10,
            *[outs[name][0] for name in SHARED], pa._lib._ptr(gK, dp), outs["rate_weight"][0], C.byref(done), None)
    finally:
        ctx._dev(False)
    assert st == 0 and done.value == n_steps
    for name, (_, keep) in outs.items():
        assert np.asarray(to_host(keep)).ravel().tobytes() == want[name].tobytes(), name
    assert gK.tobytes() == want["rate_matrix"].tobytes()
