"""Cases of the reactive transport step (pfv_transport_advance_react, ``Upwind.advance_reactive_components``), shared by
the emulation suite (test_react_emulation.py) and the GPU suite (test_gpu_react.py): each takes the library to run on.

Judges (they never touch the call under test): scipy's sparse direct solve of the whole (k Nc) system
``diag(acc_a) + w_a A`` on the diagonal blocks and ``diag(rho) K_ab`` between them, with ``A`` and ``b_ref_a`` as
``assemble_matrix_rhs`` exports them; on the 1-D line the cell-by-cell recursion with ``numpy.linalg.solve`` per cell;
``advance_components`` and ``advance`` with ``precond="sweep"`` where the step reduces to them.

The bounds are the project's: 1e-12 of max|judge| for the direct sweep, 1e-10 for a cyclic core, 1e-13 on the line."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla

import porepy_amd as pa
from tests import _upwind_cases as UP
from tests._multi_cases import components, discretized
from tests._saturation_cases import cfl_accumulation, inflow_values
from tests._satcomp_cases import plan_launches
from tests._sweep_cases import cyclic_field, edges, env, flow_order, rotation
from tests._upwind_cases import KW, data_for, line_grid, tets


# ---- rate matrices ---------------------------------------------------------------------------------------------------
def chain_with_partner(l0=0.8, l1=0.5, l2=0.1, kf=0.6, kb=0.3):
    """k = 4: the chain 0 -> 1 -> 2 (2 decays on, out of the system) plus the exchange 0 <-> 3; 3 is the immobile partner.
    K[0, 0] = l0 + kf against -l0 and -kf: its column sums to zero up to rounding."""
    K = np.zeros((4, 4))
    K[0, 0], K[1, 0], K[3, 0] = l0 + kf, -l0, -kf
    K[1, 1], K[2, 1] = l1, -l1
    K[2, 2] = l2
    K[3, 3], K[0, 3] = kb, -kb
    return K, np.array([1.0, 1.0, 1.0, 0.0])


def reversible_three():
    """k = 3: A <-> B -> C, all mobile, the last one slower"""
    K = np.array([[0.9, -0.4, 0.0], [-0.9, 0.4 + 0.7, 0.0], [0.0, -0.7, 0.0]])
    return K, np.array([1.0, 1.0, 0.5])


def random_network(k, seed=3):
    """a dense admissible K: non-positive off-diagonal entries, the diagonal their column sum plus a decay"""
    rng = np.random.default_rng(seed)
    K = -rng.random((k, k)) * (rng.random((k, k)) < 0.5)
    np.fill_diagonal(K, 0.0)
    np.fill_diagonal(K, -K.sum(axis=0) + 0.3 * rng.random(k))
    return K


def network(k):
    if k == 4:
        return chain_with_partner()
    if k == 3:
        return reversible_three()
    w = np.ones(k)
    w[k - 1], w[1] = 0.0, 0.25
    return random_network(k), w


# ---- the judge ---------------------------------------------------------------------------------------------------------
def judge(up, g, q, bc, acc, bv, c0, source, K, w, rho, n_steps):
    """spsolve of the whole system, component-major unknowns, n_steps times"""
    k, nc = c0.shape
    A, bref = None, np.zeros((k, nc))
    for a in range(k):
        if w[a] > 0 or A is None:  # (the boundary values of an immobile component are not read)
            Aa, ba = up.assemble_matrix_rhs(g, data_for(q, bc, bv[a] if w[a] > 0 else np.zeros(g.num_faces)))
            A = sps.csr_matrix(Aa)
            if w[a] > 0:
                bref[a] = ba
    R = sps.diags(np.ones(nc) if rho is None else rho)
    blocks = [[(sps.diags(acc[a]) + w[a] * A + K[a, a] * R) if a == b else K[a, b] * R for b in range(k)] for a in range(k)]
    M = sps.bmat(blocks, format="csc")
    solve = spla.splu(M).solve
    src = np.zeros((k, nc)) if source is None else source
    c = c0.copy()
    for _ in range(n_steps):
        rhs = acc * c - w[:, None] * bref + src
        c = solve(rhs.ravel()).reshape(k, nc)
        r = rhs.ravel() - M @ c.ravel()  # (one step of refinement: the judge is exact to rounding)
        c = c + solve(r).reshape(k, nc)
    return c


def rel_errs(c, ref):
    return [np.abs(c[a] - ref[a]).max() / np.abs(ref[a]).max() for a in range(ref.shape[0])]


def tets_problem(n, k, seed=5):
    g = tets(n)
    q, bc, acc, bv, c0, source = components(g, k, seed)
    K, w = network(k)
    rho = np.asarray(g.cell_volumes, dtype=float) / 0.02 * (0.5 + np.random.default_rng(seed + 1).random(g.num_cells))
    return g, q, bc, acc, bv, c0, source, K, w, rho


# ---- 1. exact against an independent judge ---------------------------------------------------------------------------
def exact(lib, n, k):
    g, q, bc, acc, bv, c0, source, K, w, rho = tets_problem(n, k)
    assert flow_order(g.num_cells, *edges(g, q))["core_cells"] == 0
    up, data = discretized(lib, g, q, bc, bv[0])
    ref = judge(up, g, q, bc, acc, bv, c0, source, K, w, rho, 3)
    # what one component reports on this handle and flux
    up.advance(g, data, c0[0], 1, acc[0], source=source[0], precond="sweep", rtol=1e-13)
    single = up.context(g).stats()
    assert single["sweep_direct_steps"] == 1
    c, info = up.advance_reactive_components(g, data, c0, 3, acc, K, rate_weight=rho, mobility=w, bc_values=bv,
                                             source=source)
    st = up.context(g).stats()
    err = rel_errs(c, ref)
    print(f"tets({n}), k = {k}: max-norm relative error per component {['%.1e' % e for e in err]}, relative residuals "
          f"{['%.1e' % r for r in info['rel_residual']]}, {st['sweep_levels']} levels, {st['sweep_launches']} launches")
    assert c.shape == (k, g.num_cells) and info["steps_done"] == 3 and info["converged"]
    assert info["iterations"] == [1] * k
    assert st["transport_react_components"] == k and st["transport_react_steps"] == 3
    assert st["transport_react_core_iterations"] == 0 and st["sweep_core_cells"] == 0
    assert st["sweep_levels"] == single["sweep_levels"] and st["sweep_launches"] == single["sweep_launches"] > 0
    assert max(err) <= 1e-12
    assert max(info["rel_residual"]) <= 1e-13
    assert min(np.abs(ref[a]).max() for a in range(k)) > 1e-3  # (every component is there)


# ---- 2. reduces to what exists -----------------------------------------------------------------------------------------
def reduces_to_components(lib, n=4, k=3):
    g = tets(n)
    q, bc, acc, bv, c0, source = components(g, k)
    up, data = discretized(lib, g, q, bc, bv[0])
    c, info = up.advance_reactive_components(g, data, c0, 3, acc, np.zeros((k, k)), mobility=np.ones(k), bc_values=bv,
                                             source=source)
    lin, ldata = discretized(lib, g, q, bc, bv[0])
    want, linfo = lin.advance_components(g, ldata, c0, 3, acc, bc_values=bv, source=source, precond="sweep", rtol=1e-13)
    assert info["steps_done"] == 3 and linfo["steps_done"] == 3
    assert lin.context(g).stats()["transport_multi_direct_steps"] == 3
    print(f"K = 0, w = 1 against advance_components: largest difference {np.abs(c - want).max():.1e}")
    assert c.tobytes() == want.tobytes()
    # and without the optional arguments: mobility None = 1, rate_weight None = 1
    c2, _ = up.advance_reactive_components(g, data, c0, 3, acc, np.zeros((k, k)), bc_values=bv, source=source)
    assert c2.tobytes() == want.tobytes()


# ---- 3. closed form ------------------------------------------------------------------------------------------------------
def closed_form(lib):
    n, qv, dt, phi, k = 16, 0.7, 0.05, 0.3, 3
    g = line_grid(n, 2.0)
    bc = pa.BoundaryCondition(g, g.get_all_boundary_faces(), ["dir", "dir"])
    bv = np.zeros((k, g.num_faces))
    bv[0, 0] = 1.0  # the parent enters; the daughters come from it alone
    acc = np.array([(1.0 + 0.5 * a) * phi * g.cell_volumes / dt for a in range(k)])
    K = np.array([[2.0, 0.0, 0.0], [-2.0, 1.0, 0.0], [0.0, -1.0, 0.25]])
    rho = phi * np.asarray(g.cell_volumes, dtype=float) * (1.0 + 0.1 * np.arange(n))
    up, data = discretized(lib, g, qv * np.ones(g.num_faces), bc, bv[0])
    c = np.zeros((k, n))
    for _ in range(10):
        new = np.empty((k, n))
        for i in range(n):
            inflow = new[:, i - 1] if i else bv[:, 0]
            new[:, i] = np.linalg.solve(np.diag(acc[:, i] + qv) + rho[i] * K, acc[:, i] * c[:, i] + qv * inflow)
        c = new
    got, info = up.advance_reactive_components(g, data, np.zeros((k, n)), 10, acc, K, rate_weight=rho, bc_values=bv)
    st = up.context(g).stats()
    err = np.abs(got - c).max() / np.abs(c).max()
    print(f"line, chain of three: {err:.1e} of max|c|; residuals {['%.1e' % r for r in info['rel_residual']]}")
    assert info["steps_done"] == 10 and st["transport_react_steps"] == 10 and st["sweep_levels"] == n
    assert err <= 1e-13
    assert c[2].max() > 1e-3  # (the granddaughter is there, and it has no source but the chain)


# ---- 4. immobile partner -----------------------------------------------------------------------------------------------
def immobile_partner(lib, n=3):
    g, q, bc, acc, bv, c0, source, K, w, rho = tets_problem(n, 4)
    bv[3] = np.nan
    c0[3] = 0.2 + np.random.default_rng(8).random(g.num_cells)
    up, data = discretized(lib, g, q, bc, bv[0])
    ref = judge(up, g, q, bc, acc, bv, c0, source, K, w, rho, 2)
    c, info = up.advance_reactive_components(g, data, c0, 2, acc, K, rate_weight=rho, mobility=w, bc_values=bv,
                                             source=source)
    assert info["steps_done"] == 2 and np.isfinite(c).all()
    assert max(rel_errs(c, ref)) <= 1e-12
    # without reactions and sources the immobile component stays where it is
    c, info = up.advance_reactive_components(g, data, c0, 3, acc, np.zeros((4, 4)), mobility=w, bc_values=bv)
    assert info["steps_done"] == 3
    assert np.abs(c[3] - c0[3]).max() <= 1e-15 * np.abs(c0[3]).max()
    assert np.abs(c[0] - c0[0]).max() > 1e-3  # (the others move)
    # the same NaN under a mobile component is refused, with its face and component
    w2 = w.copy()
    w2[3] = 0.5
    with pytest.raises(ValueError, match=r"bc_values is not finite on face \d+, component 3$"):
        up.advance_reactive_components(g, data, c0, 1, acc, K, mobility=w2, bc_values=bv)


# ---- 5. conservation -----------------------------------------------------------------------------------------------------
def conservation(lib, n=4, k=4):
    g = tets(n)
    q, bc, acc, bv, c0, source = components(g, k)
    acc = np.broadcast_to(acc[1], acc.shape).copy()  # equal accumulation
    R = 0.1 + np.random.default_rng(9).random((k, k))  # every component turns into every other one
    np.fill_diagonal(R, 0.0)
    K = np.diag(R.sum(axis=0)) - R
    assert np.abs(K.sum(axis=0)).max() <= 1e-15
    rho = np.asarray(g.cell_volumes, dtype=float) / 0.02
    up, data = discretized(lib, g, q, bc, bv[0])
    c, info = up.advance_reactive_components(g, data, c0, 3, acc, K, rate_weight=rho, bc_values=bv, source=source)
    total, tinfo = up.advance(g, data_for(q, bc, bv.sum(axis=0)), c0.sum(axis=0), 3, acc[0], source=source.sum(axis=0),
                              precond="sweep", rtol=1e-13)
    assert info["steps_done"] == 3 and tinfo["steps_done"] == 3
    err = np.abs(c.sum(axis=0) - total).max() / np.abs(total).max()
    print(f"sum over the components against one component carrying the sum: {err:.1e}")
    assert err <= 1e-12
    assert max(np.abs(c[a] - c0[a]).max() for a in range(k)) > 1e-3


# ---- 6. positivity -------------------------------------------------------------------------------------------------------
def positivity(lib, n=4):
    for k in (4, 8):
        g, q, bc, acc, bv, c0, source, K, w, rho = tets_problem(n, k)
        assert c0.min() >= 0 and bv.min() >= 0 and source.min() >= 0
        up, data = discretized(lib, g, q, bc, bv[0])
        c, info = up.advance_reactive_components(g, data, c0, 3, acc, 50.0 * K, rate_weight=rho, mobility=w, bc_values=bv,
                                                 source=source)  # (fast reactions: the off-diagonal part is large)
        assert info["steps_done"] == 3
        print(f"k = {k}: min c = {c.min():.2e}")
        assert c.min() >= 0.0


# ---- 7. launch forms and determinism -----------------------------------------------------------------------------------
def launch_forms(lib, n=4, k=4, rows=24):
    g, q, bc, acc, bv, c0, source, K, w, rho = tets_problem(n, k)
    order = flow_order(g.num_cells, *edges(g, q))
    sizes = np.bincount(order["level"], minlength=order["levels"])
    want = plan_launches(sizes, rows)
    assert plan_launches(sizes, 512) < want < order["levels"]  # (`rows` mixes single levels and runs)
    runs = []
    for environment in ({}, {}, {"PFV_SWEEP_MERGE": 0}, {"PFV_SWEEP_MERGE_ROWS": rows}):
        with env(**environment):
            up, data = discretized(lib, g, q, bc, bv[0])
            c, info = up.advance_reactive_components(g, data, c0, 3, acc, K, rate_weight=rho, mobility=w, bc_values=bv,
                                                     source=source)
            st = up.context(g).stats()
        assert info["steps_done"] == 3
        runs.append((c, st["sweep_launches"], st["sweep_levels"]))
    print("launches per sweep (merged, merged, one per level, mixed):", [r[1] for r in runs])
    for r in runs[1:]:
        assert r[0].tobytes() == runs[0][0].tobytes()
    assert runs[2][1] == runs[2][2] == order["levels"] and runs[0][1] == plan_launches(sizes, 512)
    assert runs[3][1] == want


# ---- 8. cyclic core ------------------------------------------------------------------------------------------------------
def core_case(lib, which):
    """which: the core, or "<core>-k<k>" for the network of k components (k = 3: 256 is no multiple of k, the norms'
    partition has G = 85 rows per slot and an odd fold)"""
    which, _, kk = which.partition("-k")
    g, q = cyclic_field(12) if which == "cyclic12" else rotation(8)
    n_core = 45 if which == "cyclic12" else 64
    nc, k = g.num_cells, int(kk or 4)
    K, w = network(k)
    rng = np.random.default_rng(5)
    acc0 = cfl_accumulation(g, q, 2.0)
    acc = np.array([(1.0 + 0.5 * a) * acc0 for a in range(k)])
    rho = acc0 * (0.5 + rng.random(nc))
    bv = np.array([(0.5 + 0.25 * a) * inflow_values(g, 1.0) for a in range(k)])
    c0 = 0.2 + rng.random((k, nc))
    up, data = discretized(lib, g, q, None, bv[0])
    ref = judge(up, g, q, None, acc, bv, c0, None, K, w, rho, 3)
    c, info = up.advance_reactive_components(g, data, c0, 3, acc, K, rate_weight=rho, mobility=w, bc_values=bv, rtol=1e-12)
    st = up.context(g).stats()
    err = rel_errs(c, ref)
    print(f"{which}: {max(err):.2e} of max|judge|; core of {st['sweep_core_cells']} cells, "
          f"{st['transport_react_core_iterations']} core iterations in all, {info['iterations'][0]} in the last step, "
          f"relative residuals {['%.1e' % r for r in info['rel_residual']]}")
    assert info["steps_done"] == 3 and info["converged"] and max(info["rel_residual"]) <= 1e-12
    assert st["sweep_core_cells"] == n_core
    assert info["iterations"] == [info["iterations"][0]] * k
    assert st["transport_react_core_iterations"] >= info["iterations"][0] > 0
    assert max(err) <= 1e-10
    # two iterations are not enough: the call says so and hands the state back untouched
    c2, i2 = up.advance_reactive_components(g, data, c0, 3, acc, K, rate_weight=rho, mobility=w, bc_values=bv, rtol=1e-12,
                                            maxit=2, raise_on_fail=False)
    assert i2["steps_done"] == 0 and not i2["converged"] and i2["iterations"] == [2] * k
    assert c2.tobytes() == np.ascontiguousarray(c0).tobytes()
    with pytest.raises(pa.PorefvError) as e:
        up.advance_reactive_components(g, data, c0, 3, acc, K, rate_weight=rho, mobility=w, bc_values=bv, maxit=2)
    assert e.value.status == 6 and "did not settle in 2 iterations" in e.value.message
    assert e.value.state.tobytes() == np.ascontiguousarray(c0).tobytes() and e.value.info["steps_done"] == 0


# ---- 9. refusals ---------------------------------------------------------------------------------------------------------
def refusals(lib):
    g, q, bc, acc, bv, c0, source, K, w, rho = tets_problem(3, 4)
    nc, nf = g.num_cells, g.num_faces
    up = pa.Upwind(KW, library=lib)
    data = data_for(q, bc, bv[0])
    args = dict(rate_weight=rho, mobility=w, bc_values=bv, source=source)
    # before discretize
    with pytest.raises((ValueError, pa.PorefvError)):
        up.advance_reactive_components(g, data, c0, 1, acc, K, **args)
    up.discretize(g, data)
    ctx = up.context(g)
    # k = 0 and k = 9, at both levels
    dp, ptr = pa._lib._dp, pa._lib._ptr
    for k in (0, 9):
        with pytest.raises(ValueError, match=rf"1 \.\. 8, not {k} "):
            up.advance_reactive_components(g, data, np.zeros((k, nc)), 1, np.ones(nc), np.zeros((k, k)))
        m = max(k, 1)
        st = ctx.lib.pfv_transport_advance_react(ctx._h, None, k, ptr(np.zeros(m * nf), dp), ptr(np.ones(m * nc), dp), None,
                                                 None, ptr(np.zeros(m * m), dp), None, 1, 1e-12, 10,
                                                 ptr(np.zeros(m * nc), dp), None, None)
        assert st == 4 and f"k = {k}" in ctx.lib.pfv_last_error(ctx._h).decode()

    def refused(match, **change):
        a = dict(args, acc=acc, K=K, c0=c0)
        a.update(change)
        acc_, K_, c0_ = a.pop("acc"), a.pop("K"), a.pop("c0")
        with pytest.raises(ValueError, match=match):
            up.advance_reactive_components(g, data, c0_, 1, acc_, K_, **a)

    def changed(x, idx, v):
        y = np.array(x, dtype=float, copy=True)
        y[idx] = v
        return y

    refused(r"rate\[2\]\[2\] is negative", K=changed(K, (2, 2), -0.1))
    refused(r"rate\[1\]\[3\] is positive", K=changed(K, (1, 3), 0.1))
    refused(r"column 1 of rate has a negative sum", K=changed(K, (2, 1), -0.5 - 1e-9))
    refused(r"rate\[0\]\[3\] is not finite", K=changed(K, (0, 3), np.nan))
    refused(r"rate\[0\]\[1\] is not finite", K=changed(changed(K, (0, 1), np.inf), (3, 3), -1.0))  # (the first offender)
    refused(r"mobility\[1\] is negative", mobility=changed(w, 1, -1.0))
    refused(r"mobility\[2\] is not finite", mobility=changed(w, 2, np.inf))
    refused(r"rate_weight must not be negative: cell 7$", rate_weight=changed(changed(rho, 7, -1.0), 30, -1.0))
    refused(r"rate_weight must not be negative: cell 5$", rate_weight=changed(rho, 5, np.nan))
    refused(r"accumulation must be positive: cell 11, component 2$", acc=changed(changed(acc, (2, 11), 0.0), (0, 40), 0.0))
    refused(r"accumulation must be positive: cell 4, component 1$", acc=changed(acc, (1, 4), np.nan))
    refused(r"c is not finite in cell 9, component 1$", c0=changed(changed(c0, (1, 9), np.nan), (0, 10), np.inf))
    # rounding in a column sum is not a refusal: K[0, 0] = kf + l0 against -kf and -l0
    K2, _ = chain_with_partner(l0=0.1, kf=0.7)
    c, info = up.advance_reactive_components(g, data, c0, 1, acc, K2, **args)
    assert info["steps_done"] == 1
    Kr = np.array([[0.1 + 0.2, 0.0, 0.0], [-0.1, 0.0, 0.0], [-0.2, 0.0, 0.0]])
    assert Kr[:, 0].sum() != 0.0  # (0.30000000000000004 - 0.1 - 0.2)
    c, info = up.advance_reactive_components(g, data, c0[:3], 1, acc[:3], Kr, bc_values=bv[:3])
    assert info["steps_done"] == 1
    # shapes, named
    with pytest.raises(ValueError, match=r"rate_matrix must have shape \(4, 4\), not \(3, 3\)"):
        up.advance_reactive_components(g, data, c0, 1, acc, np.zeros((3, 3)))
    with pytest.raises(ValueError, match=r"mobility must have shape \(4,\)"):
        up.advance_reactive_components(g, data, c0, 1, acc, K, mobility=np.ones(3))
    # two components in the discretization: nothing to share
    up2 = pa.Upwind(KW, library=lib)
    d2 = data_for(q, bc, bv[0], k=2)
    up2.discretize(g, d2)
    with pytest.raises(ValueError, match="num_components = 1"):
        up2.advance_reactive_components(g, d2, c0, 1, acc, K, **args)
    # periodic grid
    gp = UP.geo(pa.CartGrid([3, 3], [1.0, 1.0]))
    gp.periodic_face_map = np.vstack([np.flatnonzero(np.isclose(gp.face_centers[0], 0.0)),
                                      np.flatnonzero(np.isclose(gp.face_centers[0], 1.0))])
    with pytest.raises(pa.PorefvError) as e:
        pa.Upwind(KW, library=lib).advance_reactive_components(
            gp, data_for(np.ones(gp.num_faces), None, np.zeros(gp.num_faces)), np.zeros((2, 9)), 1, np.ones(9), np.zeros((2, 2)))
    assert e.value.status == 5
    # the inflow-face rule: a Robin face that has outflow in the discretization, inflow in the flux of the call
    bf = g.get_all_boundary_faces()
    sign = np.asarray(sps.csr_matrix(g.cell_faces)[bf].sum(axis=1)).ravel()
    outflow = bf[q[bf] * sign > 0]
    kinds = np.array(["dir"] * bf.size, dtype=object)
    kinds[np.isin(bf, outflow[:2])] = "rob"
    rob = pa.BoundaryCondition(g, bf, list(kinds))
    up.discretize(g, data_for(q, rob, bv[0]))
    c, info = up.advance_reactive_components(g, data_for(q, rob, bv[0]), c0, 1, acc, K, **args)
    assert info["steps_done"] == 1
    with pytest.raises(ValueError, match=rf"face {outflow[:2].min()}$"):
        up.advance_reactive_components(g, data_for(-q, rob, bv[0]), c0, 1, acc, K, **args)


# ---- the handle ----------------------------------------------------------------------------------------------------------
def handle(lib, n=3, k=4):
    g, q, bc, acc, bv, c0, source, K, w, rho = tets_problem(n, k)
    up, data = discretized(lib, g, q, bc, bv[0])
    ctx = up.context(g)
    args = dict(rate_weight=rho, mobility=w, bc_values=bv, source=source)
    # a system assembled before the call is not left behind for solve, nor is one of the call's own
    up.solve(g, data, accumulation=acc[0], c_old=c0[0])  # (Jacobi: the handle has no order yet)
    c, info = up.advance_reactive_components(g, data, c0, 2, acc, K, **args)
    assert ctx.stats()["sweep_order_ms"] > 0  # (built whatever preconditioner is selected)
    assert ctx.active_size() == 0
    with pytest.raises(RuntimeError):
        ctx.solve(precond="sweep")
    # the same flux again: the order is kept, the result is the same; n_steps = 0 hands c0 back
    c2, _ = up.advance_reactive_components(g, data, c0, 2, acc, K, **args)
    assert ctx.stats()["sweep_order_ms"] == 0 and c2.tobytes() == c.tobytes()
    c3, i3 = up.advance_reactive_components(g, data, c0, 0, acc, K, **args)
    assert i3["steps_done"] == 0 and c3.tobytes() == np.ascontiguousarray(c0).tobytes()
    # a single advance on this handle afterwards: the bits of a fresh handle
    one, _ = up.advance(g, data, c0[0], 3, acc[0], source=source[0], precond="sweep", rtol=1e-13)
    fresh, fdata = discretized(lib, g, q, bc, bv[0])
    want, _ = fresh.advance(g, fdata, c0[0], 3, acc[0], source=source[0], precond="sweep", rtol=1e-13)
    assert one.tobytes() == want.tobytes()
    # the C call with NULL for everything optional
    dp, ptr = pa._lib._dp, pa._lib._ptr
    cc = np.ascontiguousarray(c0).copy()
    done = C.c_int32(-1)
    st = ctx.lib.pfv_transport_advance_react(ctx._h, None, k, ptr(np.ascontiguousarray(bv), dp),
                                             ptr(np.ascontiguousarray(acc), dp), None, None,
                                             ptr(np.ascontiguousarray(K), dp), None, 1, 1e-12, 10, ptr(cc, dp),
                                             C.byref(done), None)
    assert st == 0 and done.value == 1 and ctx.stats()["transport_react_steps"] == 1
