"""Cases of the adjoint of the flow solve (pfv_flow_adjoint, ``Mpfa.adjoint_flow`` / ``Tpfa.adjoint_flow``), shared by
the emulation suite (test_flow_adjoint_emulation.py) and the GPU suite (test_gpu_flow_adjoint.py): each takes the
library to run on.

The judge is numpy and scipy and never calls the new code.  It takes ``flux`` and ``bound_flux`` from the handle
(``ctx.matrix``; pinned to the reference by the existing fixtures), forms ``A = div @ flux``, solves ``A^T mu`` by a
sparse LU with one step of refinement, and evaluates

    z = g_q - cell_faces mu,   grad_source = mu,   grad_bc_values = bound_flux^T z,
    grad_perm[r][s][c] = sum_{e=(c,f)} z_f w_f dt_f/dK_rs(c)

with its own restatement of t_e, t_f, dt_f/dK and w_f (``half_faces``, ``face_weight``).  The formulas themselves are
checked against central differences of the judge's own TPFA forward solve (``judge_against_differences``).

Figures measured with these inputs, on the emulation build and on an MI355X:

- ``judge_against_differences`` (tets(3), Tpfa restatement with a vector source, all nine entries of every seventh
  cell, h = 1e-4): worst deviation of grad_perm 7.7e-10 of its largest entry; grad_bc_values and grad_source (J is
  affine in them) 2.3e-15.  DIFF_BOUND is ten times the first.
- split check, every grid and both discretizations: worst deviation from the judge's formulas at the library's mu,
  relative to the sum of the absolute values of the terms added up: emulation 3.2e-17 (grad_perm; grad_bc_values equal
  to the last bit), MI355X 3.5e-17 (grad_perm) and 2.3e-16 (grad_bc_values, the lanes' partial sums).  The bound is the
  issue's 1e-13; the residual of the transposed system stays below 1e-13 at rtol = 1e-13 (bound 10 rtol).
- whole call against the judge's own mu, max-norm relative error per gradient: worst 3.0e-12 over all cases on the
  emulation build (Mpfa on tets(3), the defaults rtol = 1e-12 and AMG; the same figure on the MI355X).  WHOLE_BOUND is
  ten times that, far below the 1e-8 above which the solve or a formula would be wrong.
- the composed chain on CartGrid([6, 5]): 3.0e-15 against the judge's scipy chain; min |q_f| over the largest flux
  change under the perturbations 6.5e3 (required: at least 100); difference quotient (h = 1e-4) against the chain's
  grad_perm 1.2e-9 of its largest entry, bound DIFF_BOUND."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sps

import porepy_amd as pa
from porepy_amd import _lib
from tests import _adjoint_cases as AJ
from tests import _upwind_cases as UP
from tests._react_adjoint_cases import refined
from tests._upwind_cases import KW, geo, line_grid, tets

SPLIT_BOUND = 1e-13        # the issue's
DIFF_BOUND = 10 * 7.7e-10  # ten times the worst value judge_against_differences reports
WHOLE_BOUND = 10 * 3.0e-12  # ten times the worst whole-call error over all cases on the emulation build
ALL = ("permeability", "bc_values", "source", "multiplier")
GRADS = ("permeability", "bc_values", "source")

GRIDS = {
    "line7": lambda: line_grid(7, 2.0),
    "cart6x5": lambda: geo(pa.CartGrid([6, 5])),
    "tets2": lambda: tets(2),
    "tets3": lambda: tets(3),
}
# every grid with the discretizations that cover it (1-D: TPFA only, as in the reference)
COMBOS = [("line7", "tpfa"), ("cart6x5", "tpfa"), ("cart6x5", "mpfa"), ("tets2", "tpfa"), ("tets2", "mpfa"),
          ("tets3", "tpfa"), ("tets3", "mpfa")]


@functools.lru_cache(maxsize=None)
def grid(name):
    return GRIDS[name]()


def tensor(values):
    t = pa.SecondOrderTensor(np.ones(values.shape[2]))
    t.values = np.ascontiguousarray(values, dtype=float)
    return t


def spd_field(nc, rng):
    """a full symmetric positive definite tensor per cell, (3, 3, Nc)"""
    M = rng.standard_normal((nc, 3, 3))
    K = np.einsum("cij,ckj->cik", M, M) / 3.0 + np.eye(3)[None]
    return np.ascontiguousarray(K.transpose(1, 2, 0))


def flow_class(scheme):
    return pa.Mpfa if scheme == "mpfa" else pa.Tpfa


def handle(flow, g):
    """the device handle behind a flow discretization of g (Mpfa hands 1-D grids to its Tpfa object)"""
    return flow._tpfa().context(g) if (isinstance(flow, pa.Mpfa) and g.dim < 2) else flow.context(g)


def problem(lib, name, scheme, seed=5, vector_source=False):
    """Random SPD K, Dirichlet on the two sides x = min / max, Neumann elsewhere with non-zero data, a non-zero source,
    the library's forward solution and random loads."""
    g = grid(name)
    rng = np.random.default_rng(seed)
    nc, nf = g.num_cells, g.num_faces
    K = spd_field(nc, rng)
    bf = g.get_all_boundary_faces()
    x = g.face_centers[0, bf]
    on_dir = np.isclose(x, x.min()) | np.isclose(x, x.max())
    bc = pa.BoundaryCondition(g, bf, ["dir" if d else "neu" for d in on_dir])
    bv = np.zeros(nf)
    bv[bf] = np.where(on_dir, 1.0 + rng.random(bf.size), 0.2 * g.face_areas[bf] * rng.standard_normal(bf.size))
    source = g.cell_volumes * rng.standard_normal(nc)
    pars = {"second_order_tensor": tensor(K), "bc": bc, "bc_values": bv}
    vs = None
    if vector_source:
        vs = 0.3 * rng.standard_normal(nc * g.dim)
        pars["vector_source"] = vs
    data = pa.initialize_data({}, "flow", pars)
    flow = flow_class(scheme)("flow", library=lib)
    flow.discretize(g, data)
    P = dict(g=g, K=K, bc=bc, bv=bv, source=source, vs=vs, data=data, flow=flow, scheme=scheme, name=name,
             gq=rng.standard_normal(nf), gp=rng.standard_normal(nc))
    P["p"], info = flow.solve(g, data, source=source, rtol=1e-13, method="bicgstab")
    assert info["converged"]
    return P


def adjoint(P, loads="both", want=ALL, **kw):
    args = dict(grad_flux=P["gq"] if loads in ("both", "flux") else None,
                grad_pressure=P["gp"] if loads in ("both", "pressure") else None, want=want)
    args.update(kw)
    return P["flow"].adjoint_flow(P["g"], P["data"], P["p"], **args)


# ---- the judge --------------------------------------------------------------------------------------------------------
def half_faces(g, K):
    """The judge's restatement of t_e, t_f and dt_f/dK_rs(c) per half-face e = (c, f): t_e = d^T K (sgn n) / |d|^2 with
    d = x_f - x_c, t_f = 1 / sum_e 1 / t_e, dt_f/dK_rs(c) = t_f^2 d_r (sgn n_s) / (t_e^2 |d|^2)."""
    fi, ci, sg = sps.find(sps.csc_matrix(g.cell_faces))
    d = g.face_centers[:, fi] - g.cell_centers[:, ci]
    n = g.face_normals[:, fi] * sg
    dist = (d * d).sum(axis=0)
    te = np.einsum("re,rse,se->e", d, K[:, :, ci], n) / dist
    tf = 1.0 / np.bincount(fi, weights=1.0 / te, minlength=g.num_faces)
    dt = (tf[fi] ** 2 / (te ** 2 * dist))[None, None, :] * d[:, None, :] * n[None, :, :]
    return fi, ci, sg, d, tf, dt


def face_weight(g, bc, fi, ci, sg, d, p, bv, vs):
    """w_f = filter_f (p_diff_f + g_diff_f) - dir_f sgn_f bc_f and the sum of the absolute values of its terms"""
    nf, nc = g.num_faces, g.num_cells
    proj = np.zeros(fi.size) if vs is None else (d[:g.dim] * vs.reshape(nc, g.dim).T[:, ci]).sum(axis=0)
    aproj = np.zeros(fi.size) if vs is None else np.abs(d[:g.dim] * vs.reshape(nc, g.dim).T[:, ci]).sum(axis=0)
    diff = np.bincount(fi, weights=sg * (p[ci] + proj), minlength=nf)
    adiff = np.bincount(fi, weights=np.abs(p[ci]) + aproj, minlength=nf)
    bnd = np.bincount(fi, minlength=nf) == 1
    sgn = np.bincount(fi, weights=sg, minlength=nf) * bnd
    is_dir = np.asarray(bc.is_dir, dtype=bool) & bnd
    filt = np.where(bnd & ~is_dir, 0.0, 1.0)
    return filt * diff - is_dir * sgn * bv, filt * adiff + is_dir * np.abs(bv)


def matrices(P):
    """(cf, T, B, A) with flux and bound_flux as the handle exports them"""
    ctx = handle(P["flow"], P["g"])
    cf = sps.csr_matrix(P["g"].cell_faces)
    T = sps.csr_matrix(ctx.matrix(_lib.MAT_FLUX))
    B = sps.csr_matrix(ctx.matrix(_lib.MAT_BOUND_FLUX))
    return cf, T, B, (cf.T @ T).tocsr()


def formulas(P, mu, gq, K=None):
    """The three gradients at a given multiplier and, per entry, the sum of the absolute values of the terms added up."""
    g = P["g"]
    cf, T, B, _ = matrices(P)
    gq = np.zeros(g.num_faces) if gq is None else gq
    fi, ci, sg, d, tf, dt = half_faces(g, P["K"] if K is None else K)
    w, aw = face_weight(g, P["bc"], fi, ci, sg, d, P["p"], P["bv"], P["vs"])
    z = gq - cf @ mu
    az = np.abs(gq) + abs(cf) @ np.abs(mu)
    gk, ak = np.zeros((3, 3, g.num_cells)), np.zeros((3, 3, g.num_cells))
    for r in range(3):
        for s in range(3):
            gk[r, s] = np.bincount(ci, weights=(z * w)[fi] * dt[r, s], minlength=g.num_cells)
            ak[r, s] = np.bincount(ci, weights=(az * aw)[fi] * np.abs(dt[r, s]), minlength=g.num_cells)
    grads = {"permeability": gk, "bc_values": B.T @ z, "source": mu.copy(), "multiplier": mu.copy()}
    scales = {"permeability": ak, "bc_values": abs(B).T @ az, "source": np.abs(mu), "multiplier": np.abs(mu)}
    return grads, scales, z


def right_hand_side(P, loads="both"):
    _, T, _, _ = matrices(P)
    rhs = np.zeros(P["g"].num_cells)
    if loads in ("both", "flux"):
        rhs = rhs + T.T @ P["gq"]
    if loads in ("both", "pressure"):
        rhs = rhs + P["gp"]
    return rhs


def judged(P, loads="both"):
    """the judge's own gradients: mu by a sparse LU with one step of refinement"""
    _, _, _, A = matrices(P)
    mu = refined(A.T.tocsc())(right_hand_side(P, loads))
    grads, _, _ = formulas(P, mu, P["gq"] if loads in ("both", "flux") else None)
    return grads


def scaled_errors(got, ref, scales, names):
    """largest deviation per gradient relative to the sum of the absolute values of the terms added up"""
    out = {}
    for m in names:
        diff, sc = np.abs(got[m] - ref[m]), scales[m]
        assert np.all(diff[sc == 0.0] == 0.0), m  # (nothing added up: the entry is an exact zero)
        out[m] = float((diff[sc > 0.0] / sc[sc > 0.0]).max()) if np.any(sc > 0.0) else 0.0
    return out


def relative_errors(got, ref, names):
    return {m: float(np.abs(got[m] - ref[m]).max() / np.abs(ref[m]).max()) for m in names}


# ---- the judge's own TPFA forward solve (for the difference quotients) ---------------------------------------------------
def tpfa_numpy(g, K, bc):
    """(T, B, V) of the two-point scheme from the judge's t_f: flux rows zero on Neumann faces, bound_flux -t_f sgn_f on
    Dirichlet and sgn_f on Neumann faces, vector_source t_f sgn_e d per half-face."""
    nf, nc = g.num_faces, g.num_cells
    fi, ci, sg, d, tf, _ = half_faces(g, K)
    bnd = np.bincount(fi, minlength=nf) == 1
    sgn = np.bincount(fi, weights=sg, minlength=nf) * bnd
    is_dir = np.asarray(bc.is_dir, dtype=bool) & bnd
    is_neu = bnd & ~is_dir
    t = np.where(is_neu, 0.0, tf)
    T = sps.csr_matrix((t[fi] * sg, (fi, ci)), shape=(nf, nc))
    B = sps.diags(np.where(is_dir, -tf * sgn, np.where(is_neu, sgn, 0.0))).tocsr()
    rows = np.repeat(fi, g.dim)
    cols = (g.dim * ci[:, None] + np.arange(g.dim)[None, :]).ravel()
    V = sps.csr_matrix(((t[fi] * sg * d[:g.dim]).T.ravel(), (rows, cols)), shape=(nf, g.dim * nc))
    return T, B, V


def forward_numpy(g, K, bc, bv, source, vs):
    """(p, q) of the judge's TPFA problem"""
    T, B, V = tpfa_numpy(g, K, bc)
    div = sps.csr_matrix(g.cell_faces).T.tocsr()
    fixed = B @ bv + (V @ vs if vs is not None else 0.0)
    p = refined((div @ T).tocsc())(source - div @ fixed)
    return p, T @ p + fixed


def judge_against_differences(name="tets3", h=1e-4, stride=7):
    """The judge's formulas against central differences of J = <g_q, q> + <g_p, p> over its own TPFA forward solve: all
    nine entries of K in every ``stride``-th cell; bc_values and source (J is affine in them) on a few entries."""
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
    vs = 0.3 * rng.standard_normal(nc * g.dim)
    gq, gp = rng.standard_normal(nf), rng.standard_normal(nc)

    def J(K_, bv_, src_):
        p, q = forward_numpy(g, K_, bc, bv_, src_, vs)
        return float(gq @ q + gp @ p)

    p, _ = forward_numpy(g, K, bc, bv, source, vs)
    T, B, _ = tpfa_numpy(g, K, bc)
    cf = sps.csr_matrix(g.cell_faces)
    mu = refined((cf.T @ T).T.tocsc())(gp + T.T @ gq)
    fi, ci, sg, d, tf, dt = half_faces(g, K)
    w, _ = face_weight(g, bc, fi, ci, sg, d, p, bv, vs)
    z = gq - cf @ mu
    gk = np.zeros((3, 3, nc))
    for r in range(3):
        for s in range(3):
            gk[r, s] = np.bincount(ci, weights=(z * w)[fi] * dt[r, s], minlength=nc)
    gb, gs = B.T @ z, mu
    worst = {"permeability": 0.0, "bc_values": 0.0, "source": 0.0}
    for c in range(0, nc, stride):
        for r in range(3):
            for s in range(3):
                Kp, Km = K.copy(), K.copy()
                Kp[r, s, c] += h
                Km[r, s, c] -= h
                fd = (J(Kp, bv, source) - J(Km, bv, source)) / (2 * h)
                worst["permeability"] = max(worst["permeability"], abs(fd - gk[r, s, c]) / np.abs(gk).max())
    for f in bf[::5]:
        e = np.zeros(nf)
        e[f] = 1.0
        fd = (J(K, bv + e, source) - J(K, bv - e, source)) / 2.0
        worst["bc_values"] = max(worst["bc_values"], abs(fd - gb[f]) / np.abs(gb).max())
    for c in range(0, nc, stride):
        e = np.zeros(nc)
        e[c] = 1.0
        fd = (J(K, bv, source + e) - J(K, bv, source - e)) / 2.0
        worst["source"] = max(worst["source"], abs(fd - gs[c]) / np.abs(gs).max())
    print(f"judge against central differences on {name} (h = {h:g}):", {m: "%.1e" % e for m, e in worst.items()})
    assert np.abs(gb[~np.isin(np.arange(nf), bf)]).max() == 0.0
    assert worst["permeability"] <= DIFF_BOUND and worst["bc_values"] <= 1e-10 and worst["source"] <= 1e-10
    return worst


# ---- 1. the split check --------------------------------------------------------------------------------------------------
def split(lib, name, scheme, vector_source=False, precond="jacobi", rtol=1e-13):
    """With the library's own mu: the residual of the transposed system, and the three gradients against the judge's
    formulas at that mu -- the kernels apart from the accuracy of the solve."""
    P = problem(lib, name, scheme, vector_source=vector_source)
    method = "cg" if scheme == "tpfa" else "bicgstab"
    grads, info = adjoint(P, rtol=rtol, precond=precond, method=method)
    assert info["converged"] and sorted(grads) == sorted(ALL)
    g = P["g"]
    assert grads["permeability"].shape == (3, 3, g.num_cells) and grads["bc_values"].shape == (g.num_faces,)
    mu = grads["multiplier"]
    _, _, _, A = matrices(P)
    rhs = right_hand_side(P)
    res = np.linalg.norm(rhs - A.T @ mu) / np.linalg.norm(rhs)
    ref, scales, _ = formulas(P, mu, P["gq"])
    err = scaled_errors(grads, ref, scales, GRADS)
    print(f"split check, {scheme} on {name}{' with a vector source' if vector_source else ''}: residual {res:.1e}, "
          f"{info['iterations']} iterations; deviation relative to the sum of absolute terms",
          {m: "%.1e" % e for m, e in err.items()})
    assert grads["source"].tobytes() == mu.tobytes()
    bf = g.get_all_boundary_faces()
    assert np.abs(grads["bc_values"][~np.isin(np.arange(g.num_faces), bf)]).max() == 0.0
    assert res <= 10 * rtol
    assert max(err.values()) <= SPLIT_BOUND
    if scheme == "tpfa":  # the judge's own two-point matrices are the handle's
        _, T, B, _ = matrices(P)
        Tn, Bn, _ = tpfa_numpy(g, P["K"], P["bc"])
        assert abs(T - Tn).max() <= 1e-13 * abs(Tn).max() and abs(B - Bn).max() <= 1e-13 * abs(Bn).max()
    return res, err


# ---- 2. the whole call against the judge's own mu ------------------------------------------------------------------------
def whole(lib, name, scheme, vector_source=False):
    P = problem(lib, name, scheme, vector_source=vector_source)
    grads, info = adjoint(P)  # the defaults: rtol = 1e-12, AMG
    ref = judged(P)
    err = relative_errors(grads, ref, ALL)
    print(f"whole call, {scheme} on {name}: {info['iterations']} iterations, max-norm relative error",
          {m: "%.1e" % e for m, e in err.items()})
    assert info["converged"]
    assert WHOLE_BOUND <= 1e-8 and max(err.values()) <= WHOLE_BOUND
    return err


# ---- 3. load combinations and want subsets -------------------------------------------------------------------------------
def load_combinations(lib, name, scheme):
    P = problem(lib, name, scheme)
    kw = dict(rtol=1e-13, precond="jacobi")
    full = {}
    for loads in ("flux", "pressure", "both"):
        full[loads], info = adjoint(P, loads=loads, **kw)
        err = relative_errors(full[loads], judged(P, loads), ALL)
        print(f"loads = {loads}, {scheme} on {name}:", {m: "%.1e" % e for m, e in err.items()})
        assert info["converged"] and max(err.values()) <= WHOLE_BOUND
    assert not np.array_equal(full["flux"]["multiplier"], full["both"]["multiplier"])
    for want in (("multiplier",), ("permeability",), ("bc_values", "source"), ("source",), ()):
        got, info = adjoint(P, want=want, **kw)
        assert sorted(got) == sorted(want) and info["converged"]
        for m in want:
            assert got[m].tobytes() == full["both"][m].tobytes(), (want, m)
    with pytest.raises(ValueError, match="unknown gradient"):
        adjoint(P, want=("porosity",))


def one_dimensional_delegate(lib):
    """Mpfa hands a 1-D grid to its Tpfa object: the same bits as Tpfa itself."""
    P = problem(lib, "line7", "tpfa")
    g = P["g"]
    m = pa.Mpfa("flow", library=lib)
    m.discretize(g, P["data"])
    got, info = m.adjoint_flow(g, P["data"], P["p"], grad_flux=P["gq"], grad_pressure=P["gp"], method="cg", rtol=1e-13)
    want, _ = adjoint(P, want=GRADS, method="cg", rtol=1e-13)
    assert info["converged"]
    for name in GRADS:
        assert got[name].tobytes() == want[name].tobytes(), name


# ---- 4. determinism, the kept maps, the handle afterwards ---------------------------------------------------------------
def determinism_and_maps(lib, name="tets2"):
    P = problem(lib, name, "mpfa")
    g, flow, data = P["g"], P["flow"], P["data"]
    ctx = handle(flow, g)
    flux_before = ctx.matrix(_lib.MAT_FLUX).data.tobytes()
    base = ctx.stats()
    a, _ = adjoint(P)
    st = ctx.stats()
    assert st["flow_adjoint_calls"] == base["flow_adjoint_calls"] + 1 and st["flow_adjoint_map_builds"] == 1
    assert st["flow_adjoint_iterations"] > 0
    b, _ = adjoint(P)
    for m in ALL:
        assert a[m].tobytes() == b[m].tobytes(), m
    assert ctx.stats()["flow_adjoint_map_builds"] == 1
    # the handle: no active system, the discretization as it was, the forward solve as before
    with pytest.raises(RuntimeError, match="no assembled system"):
        ctx.solve()
    assert ctx.matrix(_lib.MAT_FLUX).data.tobytes() == flux_before
    p2, info = flow.solve(g, data, source=P["source"], rtol=1e-13, method="bicgstab")
    assert info["converged"] and p2.tobytes() == P["p"].tobytes()
    # J of ad_flux_system in the value array of the system: A is assembled afresh
    flow.ad_flux_system(g, data, P["p"], dk_dp=np.ones((3, 3, g.num_cells)), source=P["source"])
    c, _ = adjoint(P)
    for m in ALL:
        assert a[m].tobytes() == c[m].tobytes(), m
    # a new K on the same grid: the patterns are kept, and the maps with them
    K2 = spd_field(g.num_cells, np.random.default_rng(77))
    data[pa.PARAMETERS]["flow"]["second_order_tensor"] = tensor(K2)
    flow.discretize(g, data)
    P2 = dict(P, K=K2)
    P2["p"], _ = flow.solve(g, data, source=P["source"], rtol=1e-13, method="bicgstab")
    d, info = adjoint(P2)
    assert ctx.stats()["flow_adjoint_map_builds"] == 1
    err = relative_errors(d, judged(P2), ALL)
    assert info["converged"] and max(err.values()) <= WHOLE_BOUND and not np.array_equal(d["source"], a["source"])
    # pfv_set_grid: rebuilt
    ctx.set_grid(pa.grid_to_raw(g))
    flow.discretize(g, data)
    e2, _ = adjoint(P2)
    assert ctx.stats()["flow_adjoint_map_builds"] == 2
    for m in ALL:
        assert d[m].tobytes() == e2[m].tobytes(), m
    # pfv_tpfa_discretize writes its patterns in every call: the maps follow
    Pt = problem(lib, name, "tpfa")
    ct = handle(Pt["flow"], g)
    t1, _ = adjoint(Pt, method="cg")
    Pt["flow"].discretize(g, Pt["data"])
    t2, _ = adjoint(Pt, method="cg")
    assert ct.stats()["flow_adjoint_map_builds"] == 2
    for m in ALL:
        assert t1[m].tobytes() == t2[m].tobytes(), m


# ---- 5. Mpfa: grad_perm is the approximation ad_flux_system ships ---------------------------------------------------------
def consistent_with_ad_flux_system(lib, name, vector_source=False):
    """For a random direction dK: sum grad_perm o dK = z^T ((MAT_FLUX_JACOBIAN - MAT_FLUX) @ 1)."""
    P = problem(lib, name, "mpfa", vector_source=vector_source)
    g, flow = P["g"], P["flow"]
    grads, info = adjoint(P, rtol=1e-13)
    assert info["converged"]
    z = P["gq"] - sps.csr_matrix(g.cell_faces) @ grads["multiplier"]
    dK = np.random.default_rng(9).standard_normal((3, 3, g.num_cells))
    flow.ad_flux_system(g, P["data"], P["p"], dk_dp=dK, source=P["source"], flux_jacobian=True)
    ctx = handle(flow, g)
    JF, F = ctx.matrix(_lib.MAT_FLUX_JACOBIAN), ctx.matrix(_lib.MAT_FLUX)
    col = np.asarray((JF - F) @ np.ones(g.num_cells)).ravel()
    lhs, rhs = np.sum(grads["permeability"] * dK), z @ col
    scale = np.abs(grads["permeability"] * dK).sum() + np.abs(z * col).sum()
    print(f"consistency with ad_flux_system on {name}: {lhs:.15e} against {rhs:.15e}, {abs(lhs - rhs) / scale:.1e} of "
          "the sum of absolute terms")
    assert scale > 0 and abs(lhs - rhs) <= 1e-12 * scale


# ---- 6. device vectors ----------------------------------------------------------------------------------------------------
def device_vectors(lib, to_device=None, to_host=None, name="tets2", scheme="mpfa"):
    """Every vector of the call in device memory (pfv_set_vectors_on_device): the bits of the host-array call.
    ``to_device(array) -> (address, keepalive)``, ``to_host(keepalive) -> array``; the emulation build takes host
    addresses."""
    if to_device is None:
        to_device = lambda a: (a.ctypes.data, a)  # noqa: E731
        to_host = lambda a: a  # noqa: E731
    P = problem(lib, name, scheme, vector_source=True)
    g = P["g"]
    want, _ = adjoint(P)
    ctx = handle(P["flow"], g)

    def dev(a):
        return to_device(np.ascontiguousarray(a, dtype=np.float64))

    ins = [dev(P[m]) for m in ("p", "bv", "vs", "gq", "gp")]
    outs = {m: dev(np.zeros_like(want[m])) for m in ALL}
    _, info = ctx.flow_adjoint(ins[0][0], ins[1][0], ins[2][0], load_flux=ins[3][0], load_pressure=ins[4][0], want=ALL,
                               device=True, out_ptrs={m: outs[m][0] for m in ALL})
    assert info["converged"]
    for m in ALL:
        assert np.asarray(to_host(outs[m][1])).ravel().tobytes() == want[m].tobytes(), m


# ---- 7. the composed chain: adjoint_components -> adjoint_flow ----------------------------------------------------------
def chain(lib, h=1e-4, n_steps=3):
    """Tracer breakthrough against K: Tpfa flow on CartGrid([6, 5]) with Dirichlet pressure 2 - x - 0.7 y on the whole
    boundary, three implicit steps of one tracer, random loads on the concentrations -- the library's chain against the
    judge's scipy chain, and against central differences of the judge's whole forward chain."""
    g = grid("cart6x5")
    rng = np.random.default_rng(21)
    nc, nf = g.num_cells, g.num_faces
    kiso = np.exp(rng.uniform(-0.5, 0.5, nc))
    K = np.zeros((3, 3, nc))
    K[0, 0] = K[1, 1] = K[2, 2] = kiso
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)
    fbv = np.zeros(nf)
    fbv[bf] = 2.0 - g.face_centers[0, bf] - 0.7 * g.face_centers[1, bf]
    fdata = pa.initialize_data({}, "flow", {"second_order_tensor": tensor(K), "bc": bc, "bc_values": fbv})
    flow = pa.Tpfa("flow", library=lib)
    flow.discretize(g, fdata)
    p, info = flow.solve(g, fdata, rtol=1e-13)
    assert info["converged"]
    q = flow.darcy_flux(g, fdata, p)
    # transport: Dirichlet on the boundary (the default), one tracer
    tbv = np.zeros(nf)
    tbv[bf] = rng.random(bf.size)
    acc = (0.3 * g.cell_volumes / 0.4)[None]
    c0 = rng.random((1, nc))
    src = (g.cell_volumes * rng.random(nc))[None]
    loads = rng.standard_normal((n_steps, 1, nc))
    obs = np.arange(nc)
    up = pa.Upwind(KW, library=lib)
    tdata = UP.data_for(q, None, tbv)
    up.discretize(g, tdata)
    states = np.empty((n_steps + 1, 1, nc))
    states[0] = c0
    for s in range(n_steps):
        states[s + 1], ti = up.advance_components(g, tdata, states[s], 1, acc, bc_values=tbv[None], source=src,
                                                  rtol=1e-13)
        assert ti["steps_done"] == 1
    tg, ti = up.adjoint_components(g, tdata, n_steps, acc, loads, states=states, bc_values=tbv[None], want=("flux",))
    assert ti["steps_done"] == n_steps
    got, info = flow.adjoint_flow(g, fdata, p, grad_flux=tg["flux"], want=GRADS)
    assert info["converged"]
    # the judge's scipy chain: the transport adjoint of _adjoint_cases on the exported matrices, then the formulas above
    jstates, Ms = AJ.forward(up, g, q, None, acc, tbv[None], c0, src, n_steps)
    jt, _ = AJ.judge(g, tdata, q, Ms, acc, tbv[None], jstates, loads, obs)
    P = dict(g=g, K=K, bc=bc, bv=fbv, vs=None, p=p, flow=flow, gq=jt["flux"], gp=None)
    ref = judged(P, "flux")
    err = relative_errors(got, ref, GRADS)
    print("the chain against the judge's scipy chain:", {m: "%.1e" % e for m, e in err.items()})
    assert max(err.values()) <= WHOLE_BOUND
    # central differences of the judge's whole forward chain (numpy alone), valid while no face changes its upstream side
    is_dir, is_neu = UP.default_flags(g)
    div = sps.csr_matrix(g.cell_faces).T.tocsr()

    def run(K_):
        _, q_ = forward_numpy(g, K_, bc, fbv, np.zeros(nc), None)
        mats = UP.upwind_numpy(g, q_, is_dir, is_neu)
        A, bref = UP.system_numpy(g, q_, mats, tbv)
        solve = refined((sps.diags(acc[0]) + A).tocsc())
        c, J = c0[0], 0.0
        for s in range(n_steps):
            c = solve(acc[0] * c - bref + src[0])
            J += float(loads[s, 0] @ c)
        return J, q_

    _, q0 = run(K)
    assert np.abs(q0 - q).max() <= 1e-11 * np.abs(q).max()
    worst, dq = 0.0, 0.0
    for c in range(0, nc, 5):
        for r in range(g.dim):
            Kp, Km = K.copy(), K.copy()
            Kp[r, r, c] += h
            Km[r, r, c] -= h
            (Jp, qp), (Jm, qm) = run(Kp), run(Km)
            dq = max(dq, np.abs(qp - q0).max(), np.abs(qm - q0).max())
            worst = max(worst, abs((Jp - Jm) / (2 * h) - got["permeability"][r, r, c]) / np.abs(ref["permeability"]).max())
    ratio = np.abs(q0).min() / dq
    print(f"the chain against central differences (h = {h:g}): {worst:.1e}; min |q_f| / largest flux change {ratio:.1e}")
    assert ratio >= 100.0  # no face changes its upstream side under the perturbations
    assert worst <= DIFF_BOUND


# ---- 8. refusals -------------------------------------------------------------------------------------------------------
def refusals(lib):
    P = problem(lib, "tets3", "mpfa")
    g, flow, data = P["g"], P["flow"], P["data"]
    ctx = handle(flow, g)
    # no loads
    with pytest.raises(ValueError, match="grad_flux"):
        flow.adjoint_flow(g, data, P["p"])
    with pytest.raises(pa.PorefvError) as e:
        ctx.flow_adjoint(P["p"], P["bv"])
    assert e.value.status == 4 and "no loads" in e.value.message
    # a NaN in a load, in p, in a boundary value: the lowest index is named; status 4 is a ValueError one level up
    bad = P["gq"].copy()
    bad[[17, 5, 40]] = np.nan
    with pytest.raises(ValueError, match=r"load_flux\[5\]"):
        flow.adjoint_flow(g, data, P["p"], grad_flux=bad)
    badp = P["gp"].copy()
    badp[[9, 3]] = np.inf
    with pytest.raises(ValueError, match=r"load_pressure\[3\]"):
        flow.adjoint_flow(g, data, P["p"], grad_pressure=badp)
    pp = P["p"].copy()
    pp[11] = np.nan
    with pytest.raises(ValueError, match=r"p\[11\]"):
        flow.adjoint_flow(g, data, pp, grad_flux=P["gq"])
    bf = g.get_all_boundary_faces()
    bvb = P["bv"].copy()
    bvb[bf[[7, 2]]] = np.nan
    with pytest.raises(pa.PorefvError, match=rf"bc_values\[{bf[2]}\]") as e:
        ctx.flow_adjoint(P["p"], bvb, load_flux=P["gq"])
    assert e.value.status == 4
    interior = np.flatnonzero(~np.isin(np.arange(g.num_faces), bf))
    bvi = P["bv"].copy()
    bvi[interior[0]] = np.nan  # (not a boundary face: never read)
    ctx.flow_adjoint(P["p"], bvi, load_flux=P["gq"], precond="jacobi")
    # a solve that does not converge: status 6, the outputs as they were
    with pytest.raises(pa.PorefvError) as e:
        adjoint(P, maxit=1, precond="jacobi")
    assert e.value.status == 6 and not e.value.info["converged"]
    marks = {m: np.full(s, 7.5) for m, s in (("multiplier", g.num_cells), ("permeability", 9 * g.num_cells),
                                              ("bc_values", g.num_faces), ("source", g.num_cells))}
    dp = _lib._dp
    ctx._select_precond("jacobi")
    info = _lib.SolveInfo()
    st = ctx.lib.pfv_flow_adjoint(ctx._h, _lib._ptr(P["p"], dp), _lib._ptr(P["bv"], dp), None, _lib._ptr(P["gq"], dp), None,
                                  _lib.SOLVE_BICGSTAB, 1e-12, 1, 0, _lib._ptr(marks["multiplier"], dp),
                                  _lib._ptr(marks["permeability"], dp), _lib._ptr(marks["bc_values"], dp),
                                  _lib._ptr(marks["source"], dp), C.byref(info))
    assert st == 6 and info.converged == 0 and info.iterations >= 1
    assert all(np.all(a == 7.5) for a in marks.values())
    with pytest.raises(RuntimeError, match="no assembled system"):
        ctx.solve()  # (no active system after a refused call either)
    # no discretization: new parameters without a discretize call; a handle with a grid alone
    ctx.set_params(P["K"], pa.bc_flags(P["bc"]))
    with pytest.raises(pa.PorefvError) as e:
        ctx.flow_adjoint(P["p"], P["bv"], load_flux=P["gq"])
    assert e.value.status == 4 and "no flow discretization" in e.value.message
    bare = pa.Context(library=lib)
    bare.set_grid(pa.grid_to_raw(g))
    with pytest.raises(pa.PorefvError) as e:
        bare.flow_adjoint(P["p"], P["bv"], load_flux=P["gq"])
    assert e.value.status == 4 and "no flow discretization" in e.value.message
    with pytest.raises(RuntimeError, match="discretize"):
        pa.Mpfa("flow", library=lib).adjoint_flow(g, data, P["p"], grad_flux=P["gq"])
    # a Robin face, an internal-boundary face: the first one is named
    for scheme in ("mpfa", "tpfa"):
        labels = ["dir"] * bf.size
        labels[4] = labels[9] = "rob"
        rob = pa.BoundaryCondition(g, bf, labels)
        rdata = pa.initialize_data({}, "flow", {"second_order_tensor": tensor(P["K"]), "bc": rob, "bc_values": P["bv"]})
        fr = flow_class(scheme)("flow", library=lib)
        fr.discretize(g, rdata)
        with pytest.raises(pa.PorefvError, match=f"face {bf[4]} ") as e:
            fr.adjoint_flow(g, rdata, P["p"], grad_flux=P["gq"])
        assert e.value.status == 5 and "Robin" in e.value.message
        inner = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)
        inner.is_internal[[interior[6], interior[3]]] = True
        idata = pa.initialize_data({}, "flow", {"second_order_tensor": tensor(P["K"]), "bc": inner, "bc_values": P["bv"]})
        fi = flow_class(scheme)("flow", library=lib)
        fi.discretize(g, idata)
        with pytest.raises(pa.PorefvError, match=f"face {interior[3]} ") as e:
            fi.adjoint_flow(g, idata, P["p"], grad_flux=P["gq"])
        assert e.value.status == 5 and "INTERNAL" in e.value.message
    # a partial discretization: the rows of the other faces are zero
    pdata = pa.initialize_data({}, "flow", {"second_order_tensor": tensor(P["K"]), "bc": P["bc"], "bc_values": P["bv"],
                                            "specified_cells": np.array([0, 1])})
    fp = pa.Mpfa("flow", library=lib)
    fp.discretize(g, pdata)
    with pytest.raises(RuntimeError, match="discretize"):
        fp.adjoint_flow(g, pdata, P["p"], grad_flux=P["gq"])
    with pytest.raises(pa.PorefvError) as e:
        fp.context(g).flow_adjoint(P["p"], P["bv"], load_flux=P["gq"])
    assert e.value.status == 5 and "partial" in e.value.message
    # a periodic grid: NotImplementedError from the operator, status 5 from the handle
    gp = geo(pa.CartGrid([3, 3], [1.0, 1.0]))
    gp.periodic_face_map = np.vstack([np.flatnonzero(np.isclose(gp.face_centers[0], 0.0)),
                                      np.flatnonzero(np.isclose(gp.face_centers[0], 1.0))])
    bfp = gp.get_all_boundary_faces()
    yside = bfp[np.isclose(gp.face_centers[1, bfp], 0.0) | np.isclose(gp.face_centers[1, bfp], 1.0)]
    bcp = pa.BoundaryCondition(gp, yside, ["dir"] * yside.size)
    perdata = pa.initialize_data({}, "flow", {"second_order_tensor": pa.SecondOrderTensor(np.ones(gp.num_cells)),
                                              "bc": bcp, "bc_values": np.zeros(gp.num_faces)})
    for scheme in ("mpfa", "tpfa"):
        fper = flow_class(scheme)("flow", library=lib)
        fper.discretize(gp, perdata)
        with pytest.raises(NotImplementedError, match="periodic"):
            fper.adjoint_flow(gp, perdata, np.zeros(gp.num_cells), grad_pressure=np.ones(gp.num_cells))
        cper = fper.context(gp)
        with pytest.raises(pa.PorefvError) as e:
            cper.flow_adjoint(np.zeros(cper.nc), np.zeros(cper.nf), load_pressure=np.ones(cper.nc))
        assert e.value.status == 5 and "periodic" in e.value.message
