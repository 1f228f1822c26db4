"""Cases of the exact permeability gradient of the MPFA flow solve (``want="permeability_exact"`` of
``Mpfa.adjoint_flow`` / ``Tpfa.adjoint_flow`` / ``Context.flow_adjoint``, pfv_flow_adjoint_exact), shared by the
emulation suite (test_mpfa_adjoint_emulation.py) and the GPU suite (test_gpu_mpfa_adjoint.py): each takes the library to
run on.  Grids and ``problem()`` are those of _flow_adjoint_cases.py.

The judge (``exact_formulas``) is numpy and never calls the new code.  It restates, node by node, the GRADIENT form of
the interaction-region system (one gradient per sub-cell, an (nd deg)^2 system ``G g = Rc p + Rb bc +
E gamma``), not the condensed form the kernel solves.  With ``u_j = g_j - gamma_j`` and the sub-face flux
``q_s = -nK_{h*} . u_{j*}``, the multiplier of the region is ``G^T nu = -W^T z`` (W: the rows ``-nK_{h*}``,
``z_s = z_{f(s)}``, ``z = g_q - cell_faces mu``) and

    grad[r][b][c] = sum_{h = (j, s) of cell c} ( -z_s [h = h*(s)] + nu_s sgn_h [s a flux-continuity row] ) n_h[r] u_j[b]

K enters only through ``nK_h = n_h^T K_c``.

Figures measured with these inputs, on the emulation build and on an MI355X:

- ``judge_against_differences`` (central differences of J = <g_q, q> + <g_p, p> through oracle.mpfa_oracle.discretize /
  assemble_matrix_rhs and a sparse LU, h = 1e-4, every entry of K perturbed on its own): tets(3) with a vector source,
  all nine entries of every seventh cell: worst deviation 1.1e-9 of the largest gradient entry; CartGrid([6, 5]), all
  nine entries of every cell: 3.3e-9.  EXACT_DIFF_BOUND is ten times the larger, 3.3e-8 (below the 1e-7 above which
  the formula, not the step size, would be wrong).
- library against judge at the library's own mu, per entry relative to the sum of the absolute values of the terms
  added up, every Mpfa grid with and without a vector source: worst 2.5e-13 on the emulation build (tets(3); 2.9e-15
  of the largest entry), 2.2e-13 on the MI355X (3.2e-15 of the largest entry); CartGrid([6, 5]) 1.1e-14 / 7.4e-15.  The
  local solves are conditioned like the discretization's, hence not the 1e-17 of the two-point split check.
  EXACT_SPLIT_BOUND is ten times the emulation value.
- ``k_orthogonal``: diagonal entries of the exact Mpfa gradient against Tpfa's "permeability" 8.1e-15 (emulation),
  2.6e-15 (MI355X) of the sum of the absolute terms.
- ``it_matters`` on tets(3): the exact gradient and the two-point "permeability" differ by 0.479 of the largest entry,
  on both builds and by the judge alone (required: more than 100 EXACT_DIFF_BOUND = 3.3e-6).
- the composed chain on tets(2), all nine entries of every eleventh cell: 5.4e-10 (emulation) / 5.2e-10 (MI355X) against
  central differences; min |q_f| over the largest flux change 4.0e3 (required: at least 100)."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sps
import scipy.sparse.linalg as spla

import porepy_amd as pa
from oracle import mpfa_oracle as mo
from porepy_amd import _lib
from tests import _flow_adjoint_cases as FA
from tests import _upwind_cases as UP
from tests._flow_adjoint_cases import grid, handle, problem, spd_field, tensor
from tests._react_adjoint_cases import refined
from tests._upwind_cases import KW, geo

EXACT_DIFF_BOUND = 10 * 3.3e-9    # ten times the worst value judge_against_differences reports
EXACT_SPLIT_BOUND = 10 * 2.5e-13  # ten times the worst emulation value of library_against_judge
KEY = "permeability_exact"
MPFA_GRIDS = ("cart6x5", "tets2", "tets3")


# ---- the judge --------------------------------------------------------------------------------------------------------
def exact_formulas(g, K, bc, p, bv, vs, z):
    """(grad, scale): the exact gradient (3, 3, Nc) of z^T (T p + B bc + V gamma) with respect to K at fixed p, bc, gamma
    -- node by node in the gradient form --, and per entry the sum of the absolute values of the terms added up.
    Dirichlet and Neumann faces only."""
    raw = pa.grid_to_raw(g)
    nd = int(raw["dim"])
    eta = mo.default_eta(raw.get("name", ""))
    nodes, fc, cc, fnrm = raw["nodes"], raw["face_centers"], raw["cell_centers"], raw["face_normals"]
    nf, nc = fc.shape[1], cc.shape[1]
    nn_face = np.diff(raw["fn_indptr"])
    h_c, h_f, h_v, h_s = mo.sub_half_faces(raw)
    is_bnd = (np.bincount(h_f, minlength=nf) // np.maximum(nn_face, 1)) == 1
    is_dir = np.asarray(bc.is_dir, dtype=bool) & is_bnd
    gam = np.zeros((nc, nd)) if vs is None else np.asarray(vs, dtype=float).reshape(nc, nd)
    grad, scale = np.zeros((3, 3, nc)), np.zeros((3, 3, nc))
    start = np.flatnonzero(np.r_[True, h_v[1:] != h_v[:-1], True])
    for a, b in zip(start[:-1], start[1:]):
        v = h_v[a]
        hc, hf, hs = h_c[a:b], h_f[a:b], h_s[a:b]
        cells, jloc = np.unique(hc, return_inverse=True)
        faces, sloc = np.unique(hf, return_inverse=True)
        deg, nsf, nh = cells.size, faces.size, hc.size
        m = nd * deg
        n_h = fnrm[:nd, hf] / nn_face[hf]
        nK = np.einsum("ih,ijh->jh", n_h, K[:nd, :nd, hc])
        eta_h = np.where(is_bnd[hf], 0.0, eta)
        xcp = fc[:nd, hf] + eta_h * (nodes[:nd, [v]] - fc[:nd, hf])
        d_h = xcp - cc[:nd, hc]
        rows_F = [s for s in range(nsf) if not is_dir[faces[s]]]           # flux continuity / Neumann
        rows_P = [s for s in range(nsf) if not is_bnd[faces[s]] or is_dir[faces[s]]]  # potential continuity / Dirichlet
        assert len(rows_F) + len(rows_P) == m
        rF = {s: r for r, s in enumerate(rows_F)}
        rP = {s: len(rows_F) + r for r, s in enumerate(rows_P)}
        G, rhs = np.zeros((m, m)), np.zeros(m)
        for h in range(nh):
            s, j, f, sg = sloc[h], jloc[h], hf[h], hs[h]
            cols = slice(nd * j, nd * j + nd)
            if s in rF:
                G[rF[s], cols] += sg * nK[:, h]
                rhs[rF[s]] += sg * nK[:, h] @ gam[hc[h]]
                if is_bnd[f]:
                    rhs[rF[s]] += -bv[f] / nn_face[f]
            if s in rP:
                G[rP[s], cols] += sg * d_h[:, h]
                rhs[rP[s]] += -sg * p[hc[h]]
                if is_bnd[f]:
                    rhs[rP[s]] += sg * bv[f]
        sc = 1.0 / np.abs(G).sum(axis=1)
        Gs = sc[:, None] * G
        grd = np.linalg.solve(Gs, sc * rhs)
        u = grd.reshape(deg, nd) - gam[cells]
        first_h = np.full(nsf, -1)
        for h in range(nh - 1, -1, -1):
            first_h[sloc[h]] = h
        zs = z[faces]
        wz = np.zeros(m)  # W^T z
        for s in range(nsf):
            h = first_h[s]
            wz[nd * jloc[h]: nd * jloc[h] + nd] += -nK[:, h] * zs[s]
        nu = sc * np.linalg.solve(Gs.T, -wz)
        for h in range(nh):
            s, j = sloc[h], jloc[h]
            terms = []
            if first_h[s] == h:
                terms.append(-zs[s])
            if s in rF:
                terms.append(nu[rF[s]] * hs[h])
            outer = n_h[:, h][:, None] * u[j][None, :]
            grad[:nd, :nd, hc[h]] += sum(terms) * outer
            scale[:nd, :nd, hc[h]] += sum(abs(t) for t in terms) * np.abs(outer)
    return grad, scale


def judged_exact(P, loads="both"):
    """the judge's own exact gradient: mu by a sparse LU with one step of refinement on the handle's matrices"""
    cf, _, _, A = FA.matrices(P)
    mu = refined(A.T.tocsc())(FA.right_hand_side(P, loads))
    gq = P["gq"] if loads in ("both", "flux") else np.zeros(P["g"].num_faces)
    return exact_formulas(P["g"], P["K"], P["bc"], P["p"], P["bv"], P["vs"], gq - cf @ mu)[0]


# ---- 1. the judge against central differences (no library) ---------------------------------------------------------------
def oracle_forward(raw, div, K, bcraw, bv, source, vs):
    mats = mo.discretize(raw, K, bcraw)
    A, b = mo.assemble_matrix_rhs(raw, mats, bv, vs)
    p = spla.splu(A.tocsc()).solve(source + b)
    q = mats["flux"] @ p + mats["bound_flux"] @ bv
    if vs is not None:
        q = q + mats["vector_source"] @ vs
    return p, q, mats


ALL_ENTRIES = tuple((r, s) for r in range(3) for s in range(3))


@functools.lru_cache(maxsize=None)
def difference_problem(name, vector_source):
    """The problem of ``judge_against_differences`` and the judge's gradient at it: computed once per grid, shared by the
    cases that difference one entry of K each, and left unchanged."""
    g = grid(name)
    rng = np.random.default_rng(5)
    nc, nf = g.num_cells, g.num_faces
    K = spd_field(nc, rng)
    bf = g.get_all_boundary_faces()
    x = g.face_centers[0, bf]
    on_dir = np.isclose(x, x.min()) | np.isclose(x, x.max())
    bc = pa.BoundaryCondition(g, bf, ["dir" if d else "neu" for d in on_dir])
    bv = np.zeros(nf)
    bv[bf] = np.where(on_dir, 1.0 + rng.random(bf.size), 0.2 * g.face_areas[bf] * rng.standard_normal(bf.size))
    source = g.cell_volumes * rng.standard_normal(nc)
    vs = 0.3 * rng.standard_normal(nc * g.dim) if vector_source else None
    gq, gp = rng.standard_normal(nf), rng.standard_normal(nc)
    raw, bcraw = pa.grid_to_raw(g), pa.bc_to_raw(bc)
    div = mo.divergence(raw)

    def J(K_):
        p_, q_, _ = oracle_forward(raw, div, K_, bcraw, bv, source, vs)
        return float(gq @ q_ + gp @ p_)

    p, _, mats = oracle_forward(raw, div, K, bcraw, bv, source, vs)
    A = (div @ mats["flux"]).tocsc()
    mu = refined(A.T.tocsc())(gp + mats["flux"].T @ gq)
    gk, _ = exact_formulas(g, K, bc, p, bv, vs, gq - div.T @ mu)
    gk.setflags(write=False)
    K.setflags(write=False)
    return g, K, J, gk


def judge_against_differences(name="tets3", h=1e-4, stride=7, vector_source=True, entries=ALL_ENTRIES):
    """The judge's formula against central differences of J = <g_q, q> + <g_p, p> over the oracle's MPFA forward solve:
    the entries ``entries`` of K (all nine over the cases of a suite), each perturbed on its own, in every ``stride``-th
    cell.  One difference quotient is two whole-grid discretizations of the oracle and two sparse LUs, so the suites
    take the nine entries as nine cases of a few seconds each."""
    g, K, J, gk = difference_problem(name, vector_source)
    worst = 0.0
    for c in range(0, g.num_cells, stride):
        for r, s in entries:
            Kp, Km = K.copy(), K.copy()
            Kp[r, s, c] += h
            Km[r, s, c] -= h
            fd = (J(Kp) - J(Km)) / (2 * h)
            worst = max(worst, abs(fd - gk[r, s, c]) / np.abs(gk).max())
    print(f"exact-gradient judge against central differences on {name} (h = {h:g}), entries {list(entries)}: {worst:.1e} "
          "of the largest entry")
    if g.dim == 2:
        assert np.all(gk[2] == 0.0) and np.all(gk[:, 2] == 0.0)
    assert EXACT_DIFF_BOUND <= 1e-7 and worst <= EXACT_DIFF_BOUND
    return worst


# ---- 2. the library against the judge, at the library's own mu ---------------------------------------------------------
def exact_at_own_mu(P, **kw):
    """(grads, reference, scale) of one call that asks for the new key and the multiplier"""
    args = dict(rtol=1e-13, precond="jacobi", want=("permeability", "multiplier", KEY))
    args.update(kw)
    grads, info = FA.adjoint(P, **args)
    assert info["converged"] and grads[KEY].shape == (3, 3, P["g"].num_cells)
    z = P["gq"] - sps.csr_matrix(P["g"].cell_faces) @ grads["multiplier"]
    ref, scale = exact_formulas(P["g"], P["K"], P["bc"], P["p"], P["bv"], P["vs"], z)
    return grads, ref, scale


def library_against_judge(lib, name, vector_source=False):
    P = problem(lib, name, "mpfa", vector_source=vector_source)
    grads, ref, scale = exact_at_own_mu(P)
    err = FA.scaled_errors({KEY: grads[KEY]}, {KEY: ref}, {KEY: scale}, (KEY,))[KEY]
    print(f"exact gradient against the judge, mpfa on {name}{' with a vector source' if vector_source else ''}: "
          f"{err:.1e} of the sum of absolute terms, {np.abs(grads[KEY] - ref).max() / np.abs(ref).max():.1e} of the "
          "largest entry")
    if P["g"].dim == 2:  # only the 2 x 2 block
        assert np.all(grads[KEY][2] == 0.0) and np.all(grads[KEY][:, 2] == 0.0)
    assert err <= EXACT_SPLIT_BOUND
    return err


# ---- 3. a K-orthogonal grid: the exact MPFA gradient is the two-point one ------------------------------------------------
def k_orthogonal(lib):
    g = geo(pa.CartGrid([6, 5]))
    rng = np.random.default_rng(31)
    nc, nf = g.num_cells, g.num_faces
    K = np.zeros((3, 3, nc))
    for r in range(3):
        K[r, r] = np.exp(rng.uniform(-1.0, 1.0, nc))
    bf = g.get_all_boundary_faces()
    x = g.face_centers[0, bf]
    on_dir = np.isclose(x, x.min()) | np.isclose(x, x.max())
    bc = pa.BoundaryCondition(g, bf, ["dir" if d else "neu" for d in on_dir])
    bv = np.zeros(nf)
    bv[bf] = np.where(on_dir, 1.0 + rng.random(bf.size), 0.2 * g.face_areas[bf] * rng.standard_normal(bf.size))
    source = g.cell_volumes * rng.standard_normal(nc)
    gq, gp = rng.standard_normal(nf), rng.standard_normal(nc)
    out, flux = {}, {}
    p = None
    for scheme in ("mpfa", "tpfa"):
        data = pa.initialize_data({}, "flow", {"second_order_tensor": tensor(K), "bc": bc, "bc_values": bv})
        flow = FA.flow_class(scheme)("flow", library=lib)
        flow.discretize(g, data)
        flux[scheme] = sps.csr_matrix(handle(flow, g).matrix(_lib.MAT_FLUX))
        if p is None:
            p, info = flow.solve(g, data, source=source, rtol=1e-13, method="bicgstab")
            assert info["converged"]
        out[scheme], info = flow.adjoint_flow(g, data, p, grad_flux=gq, grad_pressure=gp, rtol=1e-13, precond="jacobi",
                                              want=("permeability", "multiplier", KEY), method="bicgstab")
        assert info["converged"]
    assert abs(flux["mpfa"] - flux["tpfa"]).max() <= 1e-12 * abs(flux["tpfa"]).max()
    z = gq - sps.csr_matrix(g.cell_faces) @ out["mpfa"]["multiplier"]
    _, scale = exact_formulas(g, K, bc, p, bv, None, z)
    worst = 0.0
    for r in range(3):
        diff = np.abs(out["mpfa"][KEY][r, r] - out["tpfa"]["permeability"][r, r])
        assert np.all(diff[scale[r, r] == 0.0] == 0.0)
        if np.any(scale[r, r] > 0.0):
            worst = max(worst, float((diff[scale[r, r] > 0] / scale[r, r][scale[r, r] > 0]).max()))
    print(f"K-orthogonal grid: diagonal entries of the exact MPFA gradient against the TPFA gradient, {worst:.1e} of the "
          "sum of absolute terms")
    assert worst <= EXACT_SPLIT_BOUND
    assert out["tpfa"][KEY].tobytes() == out["tpfa"]["permeability"].tobytes()  # TPFA: its exact gradient under both keys


# ---- 4. it matters -------------------------------------------------------------------------------------------------------
def it_matters(lib, golden=None):
    """tets(3): the exact gradient and the two-point rule differ by far more than either is uncertain; "permeability"
    keeps its bits (``golden``: the two-point gradient of this call as the library returned it before
    pfv_flow_adjoint_exact existed, or None).  The fixture tests/golden/mpfa_adjoint/two_point_permeability.npz holds one
    array per build, ``emulation`` and ``mi355x``.  Its bits depend on everything between the inputs and grad_perm: the
    MPFA discretization, the assembly of A, the AMG set-up and the BiCGStab loop that give mu (reduction orders of
    rocPRIM and of the library's own kernels, the compiler's contraction of multiply-adds), and the face and cell
    kernels of flow_adjoint.inc.  A compiler or rocPRIM update that reorders one of those sums moves the bits without
    any change to grad_perm: then compare with ``library_against_judge`` / FA.split, and record the fixture anew."""
    P = problem(lib, "tets3", "mpfa")
    # the judge alone first: its exact gradient against its own two-point formulas
    cf, _, _, A = FA.matrices(P)
    mu = refined(A.T.tocsc())(FA.right_hand_side(P))
    two_point = FA.formulas(P, mu, P["gq"])[0]["permeability"]
    exact = exact_formulas(P["g"], P["K"], P["bc"], P["p"], P["bv"], P["vs"], P["gq"] - cf @ mu)[0]
    jdiff = np.abs(exact - two_point).max() / np.abs(exact).max()
    grads, info = FA.adjoint(P, want=("permeability", KEY))
    assert info["converged"]
    diff = np.abs(grads[KEY] - grads["permeability"]).max() / np.abs(grads[KEY]).max()
    print(f"tets3: exact gradient against the two-point rule, {diff:.2e} of the largest entry (the judge alone: {jdiff:.2e})")
    assert jdiff > 100 * EXACT_DIFF_BOUND and diff > 100 * EXACT_DIFF_BOUND
    alone, _ = FA.adjoint(P, want=("permeability",))
    assert alone["permeability"].tobytes() == grads["permeability"].tobytes()
    if golden is not None:
        assert grads["permeability"].tobytes() == np.ascontiguousarray(golden).tobytes()
    return grads["permeability"]


# ---- 5. the composed chain ----------------------------------------------------------------------------------------------
def chain(lib, h=1e-4, n_steps=3):
    """Tracer breakthrough against K through the MPFA flow on tets(2): discretize -> solve -> darcy_flux(resident) ->
    advance_components -> adjoint_components -> adjoint_flow(want="permeability_exact"), against central differences of
    the judge's whole forward chain (the oracle's MPFA, numpy upwind)."""
    g = grid("tets2")
    rng = np.random.default_rng(21)
    nc, nf = g.num_cells, g.num_faces
    k = 1 + rng.random(nc)
    K = np.zeros((3, 3, nc))
    K[0, 0], K[1, 1], K[2, 2] = k, 1.5 * k, 0.7 * k
    K[0, 1] = K[1, 0] = 0.1 * k
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)
    fbv = np.zeros(nf)
    fbv[bf] = g.face_centers[:, bf].sum(axis=0)
    fdata = pa.initialize_data({}, "flow", {"second_order_tensor": tensor(K), "bc": bc, "bc_values": fbv})
    flow = pa.Mpfa("flow", library=lib)
    flow.discretize(g, fdata)
    p, info = flow.solve(g, fdata, rtol=1e-13)
    assert info["converged"]
    q = flow.darcy_flux(g, fdata, p)
    flow.darcy_flux(g, fdata, p, resident=True)
    up = pa.Upwind(KW, library=lib, flow=flow)
    tbv = np.zeros(nf)
    tbv[bf] = rng.random(bf.size)
    tdata = pa.initialize_data({}, KW, {"bc_values": tbv})
    up.discretize(g, tdata)
    acc = (4 * np.abs(q).max() * np.ones(nc))[None]
    c0 = rng.random((1, nc))
    src = (g.cell_volumes * rng.random(nc))[None]
    loads = rng.standard_normal((n_steps, 1, nc))
    states = np.empty((n_steps + 1, 1, nc))
    states[0] = c0
    for s in range(n_steps):
        states[s + 1], ti = up.advance_components(g, tdata, states[s], 1, acc, bc_values=tbv[None], source=src,
                                                  rtol=1e-13)
        assert ti["steps_done"] == 1
    tg, ti = up.adjoint_components(g, tdata, n_steps, acc, loads, states=states, bc_values=tbv[None], want=("flux",))
    assert ti["steps_done"] == n_steps
    got, info = flow.adjoint_flow(g, fdata, p, grad_flux=tg["flux"], want=(KEY,), rtol=1e-13)
    assert info["converged"] and sorted(got) == [KEY]
    # central differences of the judge's forward chain, valid while no face changes its upstream side
    raw, bcraw = pa.grid_to_raw(g), pa.bc_to_raw(bc)
    div = mo.divergence(raw)
    is_dir, is_neu = UP.default_flags(g)

    def run(K_):
        _, q_, _ = oracle_forward(raw, div, K_, bcraw, fbv, np.zeros(nc), None)
        mats = UP.upwind_numpy(g, q_, is_dir, is_neu)
        A, bref = UP.system_numpy(g, q_, mats, tbv)
        solve = refined((sps.diags(acc[0]) + A).tocsc())
        c, J = c0[0], 0.0
        for s in range(n_steps):
            c = solve(acc[0] * c - bref + src[0])
            J += float(loads[s, 0] @ c)
        return J, q_

    _, q0 = run(K)
    assert np.abs(q0 - q).max() <= 1e-10 * np.abs(q).max()
    worst, dq = 0.0, 0.0
    for c in range(0, nc, 11):
        for r in range(3):
            for s in range(3):
                Kp, Km = K.copy(), K.copy()
                Kp[r, s, c] += h
                Km[r, s, c] -= h
                (Jp, qp), (Jm, qm) = run(Kp), run(Km)
                dq = max(dq, np.abs(qp - q0).max(), np.abs(qm - q0).max())
                worst = max(worst, abs((Jp - Jm) / (2 * h) - got[KEY][r, s, c]) / np.abs(got[KEY]).max())
    ratio = np.abs(q0).min() / dq
    print(f"the MPFA chain against central differences (h = {h:g}): {worst:.1e}; min |q_f| / largest flux change "
          f"{ratio:.1e}")
    assert ratio >= 100.0  # no face changes its upstream side under the perturbations
    assert worst <= EXACT_DIFF_BOUND


# ---- 6. housekeeping -----------------------------------------------------------------------------------------------------
def determinism_and_map(lib, name="tets2"):
    P = problem(lib, name, "mpfa", vector_source=True)
    g, flow, data = P["g"], P["flow"], P["data"]
    ctx = handle(flow, g)
    flow.darcy_flux(g, data, P["p"], resident=True)
    flux_before = ctx.matrix(_lib.MAT_FLUX).data.tobytes()
    q_before = ctx.resident_flux().tobytes()
    base = ctx.stats()
    assert base["flow_adjoint_exact_calls"] == 0 and base["flow_adjoint_exact_map_builds"] == 0
    want = ("permeability", "bc_values", "source", "multiplier", KEY)
    a, _ = FA.adjoint(P, want=want)
    b, _ = FA.adjoint(P, want=want)
    st = ctx.stats()
    assert st["flow_adjoint_exact_calls"] == 2 and st["flow_adjoint_exact_map_builds"] == 1
    for m in want:
        assert a[m].tobytes() == b[m].tobytes(), m
    # the other outputs are those of the call without the new key
    c, _ = FA.adjoint(P, want=FA.ALL)
    assert ctx.stats()["flow_adjoint_exact_calls"] == 2
    for m in FA.ALL:
        assert a[m].tobytes() == c[m].tobytes(), m
    only, _ = FA.adjoint(P, want=(KEY,))
    assert sorted(only) == [KEY] and only[KEY].tobytes() == a[KEY].tobytes()
    # the handle: discretization and resident flux as they were, no active system, the forward solve as before
    assert ctx.matrix(_lib.MAT_FLUX).data.tobytes() == flux_before
    assert ctx.resident_flux().tobytes() == q_before
    with pytest.raises(RuntimeError, match="no assembled system"):
        ctx.solve()
    p2, info = flow.solve(g, data, source=P["source"], rtol=1e-13, method="bicgstab")
    assert info["converged"] and p2.tobytes() == P["p"].tobytes()
    # a new K on the same grid: the topology digest stands, and the map with it
    K2 = spd_field(g.num_cells, np.random.default_rng(77))
    data[pa.PARAMETERS]["flow"]["second_order_tensor"] = tensor(K2)
    flow.discretize(g, data)
    P2 = dict(P, K=K2)
    P2["p"], _ = flow.solve(g, data, source=P["source"], rtol=1e-13, method="bicgstab")
    grads, ref, scale = exact_at_own_mu(P2)
    assert ctx.stats()["flow_adjoint_exact_map_builds"] == 1
    assert FA.scaled_errors({KEY: grads[KEY]}, {KEY: ref}, {KEY: scale}, (KEY,))[KEY] <= EXACT_SPLIT_BOUND
    assert not np.array_equal(grads[KEY], a[KEY])
    # pfv_set_grid: rebuilt
    ctx.set_grid(pa.grid_to_raw(g))
    flow.discretize(g, data)
    again, _, _ = exact_at_own_mu(P2)
    assert ctx.stats()["flow_adjoint_exact_map_builds"] == 2
    assert again[KEY].tobytes() == grads[KEY].tobytes()


def tpfa_and_delegate(lib):
    """A TPFA handle returns its exact gradient under the new key; Mpfa's 1-D delegate passes the key through."""
    for name in ("tets2", "line7"):
        P = problem(lib, name, "tpfa")
        got, info = FA.adjoint(P, want=("permeability", KEY), method="cg", rtol=1e-13)
        assert info["converged"] and got[KEY].tobytes() == got["permeability"].tobytes()
        assert np.abs(got[KEY]).max() > 0.0
        assert handle(P["flow"], P["g"]).stats()["flow_adjoint_exact_calls"] == 0  # (no region pass)
    g = P["g"]
    m = pa.Mpfa("flow", library=lib)
    m.discretize(g, P["data"])
    via, info = m.adjoint_flow(g, P["data"], P["p"], grad_flux=P["gq"], grad_pressure=P["gp"], method="cg", rtol=1e-13,
                               want=(KEY,))
    assert info["converged"] and via[KEY].tobytes() == got[KEY].tobytes()


def device_vectors(lib, to_device=None, to_host=None, name="tets2"):
    """Every vector of the call in device memory (pfv_set_vectors_on_device): the bits of the host-array call."""
    if to_device is None:
        to_device = lambda a: (a.ctypes.data, a)  # noqa: E731
        to_host = lambda a: a  # noqa: E731
    P = problem(lib, name, "mpfa", vector_source=True)
    names = ("permeability", "multiplier", KEY)
    want, _ = FA.adjoint(P, want=names)
    ctx = handle(P["flow"], P["g"])

    def dev(a):
        return to_device(np.ascontiguousarray(a, dtype=np.float64))

    ins = [dev(P[m]) for m in ("p", "bv", "vs", "gq", "gp")]
    outs = {m: dev(np.zeros_like(want[m])) for m in names}
    _, info = ctx.flow_adjoint(ins[0][0], ins[1][0], ins[2][0], load_flux=ins[3][0], load_pressure=ins[4][0], want=names,
                               device=True, out_ptrs={m: outs[m][0] for m in names})
    assert info["converged"]
    for m in names:
        assert np.asarray(to_host(outs[m][1])).ravel().tobytes() == want[m].ravel().tobytes(), m


def raw_call(ctx, p, bv, gq, precond="jacobi"):
    """pfv_flow_adjoint_exact with marked outputs: (status, every mark still in place).  ``precond`` None: the
    preconditioner selected on the handle is left alone (a call from inside a running solve)."""
    marks = [np.full(s, 7.5) for s in (ctx.nc, 9 * ctx.nc, 9 * ctx.nc, ctx.nf, ctx.nc)]
    dp = _lib._dp
    if precond is not None:
        ctx._select_precond(precond)
    info = _lib.SolveInfo()
    st = ctx.lib.pfv_flow_adjoint_exact(ctx._h, _lib._ptr(p, dp), _lib._ptr(bv, dp), None, _lib._ptr(gq, dp), None,
                                        _lib.SOLVE_BICGSTAB, 1e-12, 20000, 0, *[_lib._ptr(a, dp) for a in marks],
                                        C.byref(info))
    return st, all(np.all(a == 7.5) for a in marks)


def region_too_large(lib, n=128):
    """fan_grid_3d(128): hub and pole are met by 128 faces and 64 tetrahedra.  That region fits the LDS for ``discretize``
    (151 392 bytes) but not with the exact gradient's own arrays beside it (166 240 of 163 840): refused with status 5
    naming the node, before the solve, nothing written; the other outputs of the same handle are still to be had.  (A
    2-D fan cannot get there: the symbolic phase refuses more than 127 triangles around a node, and 127 still fit.)"""
    from tests._node_class_cases import fan_grid_3d

    g = fan_grid_3d(n)
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)
    bv = np.zeros(g.num_faces)
    bv[bf] = 1.0 + g.face_centers[0, bf]
    data = pa.initialize_data({}, "flow", {"second_order_tensor": pa.SecondOrderTensor(np.ones(g.num_cells)), "bc": bc,
                                           "bc_values": bv})
    flow = pa.Mpfa("flow", library=lib)
    flow.discretize(g, data)
    p, info = flow.solve(g, data, rtol=1e-12)
    assert info["converged"]
    gq = np.ones(g.num_faces)
    ctx = flow.context(g)
    base = ctx.stats()["flow_adjoint_calls"]
    with pytest.raises(pa.PorefvError, match=r"node [01] \(up to 128 sub-faces\)") as e:
        flow.adjoint_flow(g, data, p, grad_flux=gq, want=(KEY,))
    assert e.value.status == 5 and "LDS" in e.value.message
    assert raw_call(ctx, p, bv, gq) == (5, True)
    assert ctx.stats()["flow_adjoint_calls"] == base  # (refused before its solve)
    got, info = flow.adjoint_flow(g, data, p, grad_flux=gq, want=("permeability", "source"))
    assert info["converged"] and np.abs(got["permeability"]).max() > 0.0


def refusals(lib, alloc=None):
    """The refusals of pfv_flow_adjoint hold for the new export: each returns its status and writes nothing.
    ``alloc(n) -> (address, keepalive)``: n doubles of device memory (the emulation build takes host addresses)."""
    if alloc is None:
        alloc = lambda n: (lambda a: (a.ctypes.data, a))(np.zeros(n))  # noqa: E731
    P = problem(lib, "tets3", "mpfa")
    g, data = P["g"], P["data"]
    ctx = handle(P["flow"], g)
    args = (P["p"], P["bv"], P["gq"])
    st, untouched = raw_call(ctx, *args)
    assert st == 0 and not untouched  # (the call itself goes through)
    bf = g.get_all_boundary_faces()
    interior = np.flatnonzero(~np.isin(np.arange(g.num_faces), bf))
    # a Robin face, an internal-boundary face
    labels = ["dir"] * bf.size
    labels[4] = "rob"
    inner = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)
    inner.is_internal[interior[3]] = True
    for cond, word in ((pa.BoundaryCondition(g, bf, labels), "Robin"), (inner, "INTERNAL")):
        cdata = pa.initialize_data({}, "flow", {"second_order_tensor": tensor(P["K"]), "bc": cond, "bc_values": P["bv"]})
        f = pa.Mpfa("flow", library=lib)
        f.discretize(g, cdata)
        with pytest.raises(pa.PorefvError, match=word) as e:
            f.adjoint_flow(g, cdata, P["p"], grad_flux=P["gq"], want=(KEY,))
        assert e.value.status == 5
        assert raw_call(f.context(g), *args) == (5, True)
    # a partial discretization
    pdata = pa.initialize_data({}, "flow", {"second_order_tensor": tensor(P["K"]), "bc": P["bc"], "bc_values": P["bv"],
                                            "specified_cells": np.array([0, 1])})
    fp = pa.Mpfa("flow", library=lib)
    fp.discretize(g, pdata)
    assert raw_call(fp.context(g), *args) == (5, True)
    # a periodic grid
    gp = geo(pa.CartGrid([3, 3], [1.0, 1.0]))
    gp.periodic_face_map = np.vstack([np.flatnonzero(np.isclose(gp.face_centers[0], 0.0)),
                                      np.flatnonzero(np.isclose(gp.face_centers[0], 1.0))])
    bfp = gp.get_all_boundary_faces()
    yside = bfp[np.isclose(gp.face_centers[1, bfp], 0.0) | np.isclose(gp.face_centers[1, bfp], 1.0)]
    bcp = pa.BoundaryCondition(gp, yside, ["dir"] * yside.size)
    perdata = pa.initialize_data({}, "flow", {"second_order_tensor": pa.SecondOrderTensor(np.ones(gp.num_cells)),
                                              "bc": bcp, "bc_values": np.zeros(gp.num_faces)})
    fper = pa.Mpfa("flow", library=lib)
    fper.discretize(gp, perdata)
    with pytest.raises(NotImplementedError, match="periodic"):
        fper.adjoint_flow(gp, perdata, np.zeros(gp.num_cells), grad_pressure=np.ones(gp.num_cells), want=(KEY,))
    cper = fper.context(gp)
    with pytest.raises(pa.PorefvError) as e:
        cper.flow_adjoint(np.zeros(cper.nc), np.zeros(cper.nf), load_pressure=np.ones(cper.nc), want=(KEY,))
    assert e.value.status == 5 and "periodic" in e.value.message
    assert raw_call(cper, np.zeros(cper.nc), np.zeros(cper.nf), np.ones(cper.nf)) == (5, True)
    # no loads; a solve that does not converge: the outputs as they were
    with pytest.raises(ValueError, match="grad_flux"):
        P["flow"].adjoint_flow(g, data, P["p"], want=(KEY,))
    with pytest.raises(pa.PorefvError) as e:
        FA.adjoint(P, maxit=1, precond="jacobi", want=(KEY,))
    assert e.value.status == 6
    # the unknown key stays unknown
    with pytest.raises(ValueError, match="unknown gradient"):
        FA.adjoint(P, want=("permeability_inexact",))
    # the sharded solve: the handle carries the caller's hooks only while pfv_solve_sharded runs, so the call is made from
    # one of them (one rank: nothing to exchange, nothing to sum)
    ctx.assemble(P["bv"], None, P["source"])
    seen = []

    def allreduce(_ptr, _count):
        if not seen:
            seen.append(raw_call(ctx, *args, precond=None))

    work, x = alloc(2 * ctx.nc + 8), alloc(ctx.nc)
    sinfo = ctx.solve_sharded(ctx.nc, lambda _ptr: None, allreduce, work[0], x[0], rtol=1e-8, maxit=200)
    assert seen and seen[0] == (5, True)
    assert sinfo["converged"]  # (the refused call left the running solve alone)
    # conditions per sub-face (flux has sub-face rows): Dirichlet on every boundary sub-face
    fs = pa.Mpfa("flow", library=lib)
    fs.discretize(g, data)
    cs = fs.context(g)
    cs.set_subface_bc(np.ones(cs.nsf, dtype=np.uint8))
    cs.discretize()
    with pytest.raises(pa.PorefvError, match="sub-face") as e:
        fs.adjoint_flow(g, data, P["p"], grad_flux=P["gq"], want=(KEY,))
    assert e.value.status == 5
    assert raw_call(cs, *args) == (5, True)
