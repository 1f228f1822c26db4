"""Cases of the adjoint of the advection-diffusion step (pfv_advdiff_adjoint, ``AdvectionDiffusion.adjoint``), shared by
the emulation suite (test_advdiff_adjoint_emulation.py) and the GPU suite (test_gpu_advdiff_adjoint.py): each takes the
library to run on.

The judge is numpy and scipy and never calls the new code.  ``S = diag(acc) + A`` with ``A`` from
``_advdiff_cases.host_system`` (the diffusion matrices exported from the handle, the numpy upwind),
``S^T lambda^n = g^n + acc o lambda^{n+1}`` by a sparse LU with one step of refinement, then, with
``y^n = cell_faces lambda^n`` and ``Lambda = sum_n lambda^n``,

    c0 = acc o lambda^1,  source = Lambda,  accumulation = sum_n lambda^n o (c^{n-1} - c^n),
    bc_values = -(B_D + rhs_neu + rhs_dir diag(w q))^T cell_faces Lambda,
    flux = -w sum_n y^n o cup^n,  cup^n = U c^n + rhs_dir bc,   flux_scale = (1/w) <q, flux>,
    conductivity[r][s][c] = sum_{e=(c,f)} zw_f dt_f/dK_rs(c),   zw = -sum_n y^n o w^n

with t_e, t_f, dt_f/dK of ``_flow_adjoint_cases.half_faces`` and w^n of ``face_weight`` for p = c^n.  The formulas are
checked against central differences of the judge's own host forward run (``judge_against_differences``).

Figures measured with these inputs, on the emulation build and on an MI355X:

- ``judge_against_differences`` (tets3, two-point restatement of the diffusion, N = 4, w = 1.7; differences in c0,
  source, acc, bc, q, w and all nine K entries of every seventh cell; h = 1e-5 for q, w and acc, 1e-4 for K, 1 for the
  affine ones): min |q_f| 1.9e-3 = 190 flux perturbations (required: at least 100); worst deviation relative to the
  largest entry of the gradient 1.4e-9 (flux_scale; conductivity 3.8e-10, accumulation 3.5e-10, flux 8.9e-11, the
  affine ones below 1e-13).  DIFF_BOUND is ten times the first.
- split check, every grid, both schemes, both Peclet regimes, Jacobi and AMG: worst deviation from the judge's formulas
  at the library's lambda, relative to the sum of the absolute values of the terms added up: emulation 4.3e-16
  (conductivity), MI355X 5.2e-16 (bc_values: the lanes' partial sums).  The bound is the issue's 1e-13; the residual of
  every transposed solve stays below 8.6e-14 at rtol = 1e-13 (bound 10 rtol).
- whole call against the judge's own lambda (the states the call was given are an input of both sides), max-norm
  relative error per gradient: 1.3e-12 over the sixteen ``whole`` cases at the defaults (c0, Mpfa on tets3); the worst
  over ALL cases that compare with the judge's lambda is 3.5e-11, the scalar flux_scale on tets(4) in
  ``fallback_path`` (every other gradient of that case: 1.3e-12 or less).  The same figures on both builds.
  WHOLE_BOUND is ten times the second, far below the 1e-8 above which a formula or the solve would be wrong.
- ``gmres_retry_path``: one retry per call, the gradients within 3.9e-12 of the judge's on both builds.
- Mpfa consistency: at most 3.0e-17 (emulation) / 2.8e-17 (MI355X) of the sum of the absolute terms; bound 1e-13.
- the chain on CartGrid([6, 5]): 2.0e-15 (emulation) / 1.1e-15 (MI355X) against the judge's scipy chain; min |q_f| over
  the largest flux change under the perturbations 6.5e3 (required: at least 100); difference quotient (h = 1e-4)
  against the chain's grad_perm 2.8e-9 of its largest entry on both builds, bound DIFF_BOUND."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sps

import porepy_amd as pa
from porepy_amd import _lib
from tests import _advdiff_cases as AD
from tests import _flow_adjoint_cases as FA
from tests import _upwind_cases as UP
from tests._advdiff_cases import KW
from tests._react_adjoint_cases import refined

N = 4
SPLIT_BOUND = 1e-13  # the issue's
DIFF_BOUND = 10 * 1.4e-9    # ten times the worst value judge_against_differences reports
WHOLE_BOUND = 10 * 3.5e-11  # ten times the worst whole-call error over all cases on the emulation build
ALL = _lib.Context.ADVDIFF_ADJOINT_GRADIENTS
GRADS = tuple(m for m in ALL if m != "multipliers")
# every grid with the schemes the forward class covers on it (1-D: Mpfa hands the grid to its Tpfa object)
COMBOS = [("line", "tpfa"), ("line", "mpfa"), ("quad", "tpfa"), ("quad", "mpfa"), ("tets2", "tpfa"), ("tets2", "mpfa"),
          ("tets3", "tpfa"), ("tets3", "mpfa")]
REGIMES = {"diffusive": 1.0, "advective": 1e-3}  # cell Peclet below 1; advection-dominated


@functools.lru_cache(maxsize=None)
def grid(kind):
    return AD.grid_of(kind)


# ---- the problem and the library's side ---------------------------------------------------------------------------------
def setup(lib, kind, scheme, regime="diffusive", w=1.0, rtol=1e-13, precond="amg", g=None, pr=None):
    """The forward problem of _advdiff_cases on the library, its states c^0 .. c^N and random loads on every cell."""
    g = grid(kind) if g is None else g
    pr = AD.problem(g, diffusivity=REGIMES[regime]) if pr is None else pr
    if w != 1.0:
        pr["par"]["flux_scale"] = w
    ad, data = AD.discretized(lib, g, pr, scheme)
    c, info, states = ad.advance(g, data, pr["c0"], N, pr["acc"], source=pr["src"], rtol=rtol, precond=precond,
                                 return_states=True)
    assert info["steps_done"] == N and states.shape == (N + 1, g.num_cells)
    rng = np.random.default_rng(31)
    P = dict(g=g, pr=pr, ad=ad, data=data, ctx=ad.context(g), states=states, w=w, scheme=scheme, kind=kind,
             q=np.asarray(pr["q"], dtype=float), loads=rng.standard_normal((N, g.num_cells)),
             K=np.asarray(pr["par"]["second_order_tensor"].values, dtype=float))
    return P


def adjoint(P, want=ALL, loads=None, obs=None, states="own", **kw):
    pr = P["pr"]
    st = P["states"] if isinstance(states, str) else states
    return P["ad"].adjoint(P["g"], P["data"], N, pr["acc"], P["loads"] if loads is None else loads, st, obs_cells=obs,
                           source=pr["src"], want=want, **kw)


# ---- the judge ------------------------------------------------------------------------------------------------------------
def pieces(g, bc, q, w, T_D, B_D):
    """(cf, A, Bsum, U, D): cell_faces, A = div T_D + w div diag(q) U, Bsum = B_D + rhs_neu + rhs_dir diag(w q), the
    upwind selection U and the Dirichlet-inflow selection D = rhs_dir -- the numpy upwind of _upwind_cases."""
    cf = sps.csr_matrix(g.cell_faces)
    mats = UP.upwind_numpy(g, q, np.asarray(bc.is_dir, bool), np.asarray(bc.is_neu, bool))
    U, D, Nn = mats["transport"], mats["rhs_dir"], mats["rhs_neu"]
    A = cf.T @ sps.csr_matrix(T_D) + w * (cf.T @ sps.diags(q) @ U)
    Bsum = sps.csr_matrix(B_D) + Nn + D @ sps.diags(w * q)
    return cf, sps.csr_matrix(A), sps.csr_matrix(Bsum), U, D


def scatter(g, loads, obs):
    if obs is None:
        return np.asarray(loads, dtype=float)
    out = np.zeros((loads.shape[0], g.num_cells))
    out[:, np.asarray(obs)] = loads
    return out


def multipliers(S, acc, gfull):
    """lambda^1 .. lambda^N of S^T lambda^n = g^n + acc o lambda^{n+1} by a sparse LU with one step of refinement"""
    solve = refined(sps.csc_matrix(S.T))
    n, nc = gfull.shape
    lam, nxt = np.zeros((n, nc)), np.zeros(nc)
    for k in range(n - 1, -1, -1):
        lam[k] = nxt = solve(gfull[k] + acc * nxt)
    return lam


def formulas(g, bc, bv, K, q, w, acc, Bsum, U, D, lam, states):
    """Every gradient at given multipliers and states and, per entry, the sum of the absolute values of the terms."""
    cf = sps.csr_matrix(g.cell_faces)
    acf, nc = abs(cf), g.num_cells
    n = lam.shape[0]
    Lam, aLam = lam.sum(axis=0), np.abs(lam).sum(axis=0)
    fi, ci, sg, d, tf, dt = FA.half_faces(g, K)
    sq, asq, zw, azw = (np.zeros(g.num_faces) for _ in range(4))
    gacc, aacc = np.zeros(nc), np.zeros(nc)
    for k in range(n):
        y, ay = cf @ lam[k], acf @ np.abs(lam[k])
        cn, cp = states[k + 1], states[k]
        cup = U @ cn + D @ bv
        sq += y * cup
        asq += ay * np.abs(cup)
        wn, awn = FA.face_weight(g, bc, fi, ci, sg, d, cn, bv, None)
        zw -= y * wn
        azw += ay * awn
        gacc += lam[k] * (cp - cn)
        aacc += np.abs(lam[k]) * (np.abs(cp) + np.abs(cn))
    gk, ak = np.zeros((3, 3, nc)), np.zeros((3, 3, nc))
    for r in range(3):
        for s in range(3):
            gk[r, s] = np.bincount(ci, weights=zw[fi] * dt[r, s], minlength=nc)
            ak[r, s] = np.bincount(ci, weights=azw[fi] * np.abs(dt[r, s]), minlength=nc)
    grads = {"c0": acc * lam[0], "source": Lam, "bc_values": -(Bsum.T @ (cf @ Lam)), "accumulation": gacc,
             "flux": -w * sq, "flux_scale": float(-(q @ sq)), "conductivity": gk, "multipliers": lam.copy()}
    scales = {"c0": np.abs(acc * lam[0]), "source": aLam, "bc_values": abs(Bsum).T @ (acf @ aLam), "accumulation": aacc,
              "flux": w * asq, "flux_scale": float(np.abs(q) @ asq), "conductivity": ak, "multipliers": np.abs(lam)}
    return grads, scales, zw


def handle_pieces(P):
    pr, g = P["pr"], P["g"]
    md = P["data"][pa.DISCRETIZATION_MATRICES][KW]
    cf, _, Bsum, U, D = pieces(g, pr["bc"], P["q"], P["w"], md["flux"], md["bound_flux"])
    A, b = AD.host_system(g, md, pr, q=P["q"], w=P["w"])
    return sps.csr_matrix(sps.diags(pr["acc"]) + A), b, Bsum, U, D


def judged(P, loads=None, obs=None):
    """The judge's own gradients: its own multipliers, at the states the call was given (an input of the adjoint); and
    the judge's own forward states, for the record."""
    pr, g = P["pr"], P["g"]
    S, b, Bsum, U, D = handle_pieces(P)
    solve = refined(sps.csc_matrix(S))
    states = np.empty((N + 1, g.num_cells))
    states[0] = pr["c0"]
    for k in range(N):
        states[k + 1] = solve(pr["acc"] * states[k] + b + pr["src"])
    lam = multipliers(S, pr["acc"], scatter(g, P["loads"] if loads is None else loads, obs))
    grads, _, _ = formulas(g, pr["bc"], pr["bv"], P["K"], P["q"], P["w"], pr["acc"], Bsum, U, D, lam, P["states"])
    return grads, states


def scaled_errors(got, ref, scales, names):
    out = {}
    for m in names:
        diff, sc = np.abs(np.asarray(got[m]) - np.asarray(ref[m])), np.asarray(scales[m])
        assert np.all(diff[sc == 0.0] == 0.0), m  # (nothing added up: the entry is an exact zero)
        out[m] = float((diff[sc > 0.0] / sc[sc > 0.0]).max()) if np.any(sc > 0.0) else 0.0
    return out


def relative_errors(got, ref, names):
    return {m: float(np.abs(np.asarray(got[m]) - np.asarray(ref[m])).max() / np.abs(ref[m]).max()) for m in names}


def fmt(err):
    return {m: "%.1e" % e for m, e in err.items()}


# ---- 0. the judge against central differences of its own host forward run -------------------------------------------------
def judge_against_differences(kind="tets3", stride=7):
    g = grid(kind)
    pr = AD.problem(g)
    bc, nc, nf = pr["bc"], g.num_cells, g.num_faces
    K0 = np.asarray(pr["par"]["second_order_tensor"].values, dtype=float)
    rng = np.random.default_rng(31)
    loads = rng.standard_normal((N, nc))
    X0 = dict(c0=pr["c0"], src=pr["src"], acc=pr["acc"], bv=pr["bv"], q=np.asarray(pr["q"], float), w=1.7, K=K0)

    def run(X):
        T, B, _ = FA.tpfa_numpy(g, X["K"], bc)
        _, A, Bsum, U, D = pieces(g, bc, X["q"], X["w"], T, B)
        cf = sps.csr_matrix(g.cell_faces)
        S = sps.csr_matrix(sps.diags(X["acc"]) + A)
        b = -(cf.T @ (Bsum @ X["bv"]))
        solve = refined(sps.csc_matrix(S))
        states = np.empty((N + 1, nc))
        states[0] = X["c0"]
        for k in range(N):
            states[k + 1] = solve(X["acc"] * states[k] + b + X["src"])
        return float(np.sum(loads * states[1:])), S, Bsum, U, D, states

    _, S, Bsum, U, D, states = run(X0)
    lam = multipliers(S, X0["acc"], loads)
    G, _, _ = formulas(g, bc, X0["bv"], K0, X0["q"], X0["w"], X0["acc"], Bsum, U, D, lam, states)
    hq = 1e-5
    qmin = np.abs(X0["q"]).min()
    print(f"min |q_f| = {qmin:.2e} = {qmin / hq:.0f} flux perturbations")
    assert qmin >= 100 * hq  # no face changes its upstream side under the perturbations

    def quotient(name, idx, h):
        Xp, Xm = dict(X0), dict(X0)
        if idx is None:
            Xp[name], Xm[name] = X0[name] + h, X0[name] - h
        else:
            Xp[name], Xm[name] = X0[name].copy(), X0[name].copy()
            Xp[name][idx] += h
            Xm[name][idx] -= h
        return (run(Xp)[0] - run(Xm)[0]) / (2 * h)

    bf = g.get_all_boundary_faces()
    plan = [("c0", "c0", range(0, nc, stride), 1.0), ("source", "src", range(0, nc, stride), 1.0),
            ("accumulation", "acc", range(0, nc, stride), 1e-5), ("bc_values", "bv", list(bf[::5]), 1.0),
            ("flux", "q", range(0, nf, stride), hq)]
    worst = {}
    for m, key, where, h in plan:
        worst[m] = max(abs(quotient(key, i, h) - G[m][i]) for i in where) / np.abs(G[m]).max()
    worst["flux_scale"] = abs(quotient("w", None, 1e-5) - G["flux_scale"]) / abs(G["flux_scale"])
    worst["conductivity"] = max(abs(quotient("K", (r, s, c), 1e-4) - G["conductivity"][r, s, c])
                                for c in range(0, nc, stride) for r in range(3) for s in range(3)) \
        / np.abs(G["conductivity"]).max()
    print(f"judge against central differences on {kind}:", fmt(worst))
    assert np.abs(G["bc_values"][~np.isin(np.arange(nf), bf)]).max() == 0.0
    assert max(worst.values()) <= DIFF_BOUND
    return worst


# ---- 1. the split check --------------------------------------------------------------------------------------------------
def split(lib, kind, scheme, regime="diffusive", precond="jacobi", rtol=1e-13):
    """With the library's own lambda^n: the residual of every transposed solve, and every gradient against the judge's
    formulas at those multipliers -- the kernels apart from the accuracy of the solve."""
    P = setup(lib, kind, scheme, regime, w=1.7)
    g, pr = P["g"], P["pr"]
    grads, info = adjoint(P, rtol=rtol, precond=precond)
    assert info["steps_done"] == N and info["converged"] and sorted(grads) == sorted(ALL)
    assert grads["conductivity"].shape == (3, 3, g.num_cells) and grads["multipliers"].shape == (N, g.num_cells)
    lam = grads["multipliers"]
    S, _, Bsum, U, D = handle_pieces(P)
    res = 0.0
    for k in range(N):
        rhs = P["loads"][k] + (pr["acc"] * lam[k + 1] if k + 1 < N else 0.0)
        res = max(res, np.linalg.norm(rhs - S.T @ lam[k]) / np.linalg.norm(rhs))
    ref, scales, _ = formulas(g, pr["bc"], pr["bv"], P["K"], P["q"], P["w"], pr["acc"], Bsum, U, D, lam, P["states"])
    err = scaled_errors(grads, ref, scales, GRADS)
    print(f"split check, {scheme} on {kind}, {regime}, {precond}: worst residual {res:.1e}; deviation relative to the "
          "sum of absolute terms", fmt(err))
    bf = g.get_all_boundary_faces()
    assert np.abs(grads["bc_values"][~np.isin(np.arange(g.num_faces), bf)]).max() == 0.0
    assert res <= 10 * rtol
    assert max(err.values()) <= SPLIT_BOUND
    return res, err


# ---- 2. the whole call at the defaults against the judge's own lambda --------------------------------------------------
def whole(lib, kind, scheme, regime="diffusive"):
    P = setup(lib, kind, scheme, regime, w=1.7, rtol=1e-12)
    grads, info = adjoint(P)  # the defaults: BiCGStab, AMG, rtol = 1e-12
    ref, jstates = judged(P)
    err = relative_errors(grads, ref, ALL)
    serr = np.abs(P["states"] - jstates).max() / np.abs(jstates).max()
    print(f"whole call, {scheme} on {kind}, {regime}: states {serr:.1e}; max-norm relative error", fmt(err))
    assert info["steps_done"] == N and info["converged"]
    assert WHOLE_BOUND <= 1e-8 and max(err.values()) <= WHOLE_BOUND
    return err


# ---- 3. observation subsets and want combinations ------------------------------------------------------------------------
def observations_and_wants(lib, kind="tets2", scheme="mpfa"):
    P = setup(lib, kind, scheme)
    g = P["g"]
    nc = g.num_cells
    rng = np.random.default_rng(8)
    kw = dict(rtol=1e-13, precond="jacobi")
    for obs in (np.array([nc // 3]), rng.permutation(nc)[: nc // 2], None):
        n_obs = nc if obs is None else obs.size
        every = rng.standard_normal((N, n_obs))
        only_last = np.zeros((N, n_obs))
        only_last[-1] = every[-1]
        for loads in (every, only_last):
            got, info = adjoint(P, loads=loads, obs=obs, **kw)
            ref, _ = judged(P, loads=loads, obs=obs)
            err = relative_errors(got, ref, ALL)
            print(f"{n_obs} observation cells, loads {'at every step' if loads is every else 'at the last step'}:", fmt(err))
            assert info["steps_done"] == N and max(err.values()) <= WHOLE_BOUND
    full, _ = adjoint(P, **kw)
    for m in ALL:
        got, info = adjoint(P, want=(m,), **kw)
        assert sorted(got) == [m] and info["steps_done"] == N
        assert np.asarray(got[m]).tobytes() == np.asarray(full[m]).tobytes(), m
    for want in (("c0", "source", "bc_values"), ("flux", "conductivity"), ()):
        got, info = adjoint(P, want=want, **kw)
        assert sorted(got) == sorted(want) and info["steps_done"] == N
        for m in want:
            assert np.asarray(got[m]).tobytes() == np.asarray(full[m]).tobytes(), (want, m)
    dflt, _ = adjoint(P, want=("c0", "source", "bc_values"), states=None, **kw)  # (none of the three needs states)
    for m in dflt:
        assert dflt[m].tobytes() == full[m].tobytes(), m
    with pytest.raises(ValueError, match="unknown gradient"):
        adjoint(P, want=("porosity",))


# ---- 4. bit-for-bit repeat, the kept maps, the forward run afterwards ------------------------------------------------------
def repeat_and_maps(lib, kind="tets2", scheme="mpfa"):
    P = setup(lib, kind, scheme)
    g, pr, ad, data, ctx = P["g"], P["pr"], P["ad"], P["data"], P["ctx"]
    c_before, _ = ad.advance(g, data, pr["c0"], N, pr["acc"], source=pr["src"])
    a, _ = adjoint(P)
    st = ctx.stats()
    builds = st["flow_adjoint_map_builds"]
    assert builds == 1 and st["advdiff_adjoint_steps"] == N and st["advdiff_adjoint_iterations"] > 0
    assert st["advdiff_adjoint_ms"] > 0 and st["advdiff_adjoint_accumulate_ms"] >= 0
    b, _ = adjoint(P)
    for m in ALL:
        assert np.asarray(a[m]).tobytes() == np.asarray(b[m]).tobytes(), m
    assert ctx.stats()["flow_adjoint_map_builds"] == builds
    c_after, info = ad.advance(g, data, pr["c0"], N, pr["acc"], source=pr["src"])
    assert info["steps_done"] == N and c_after.tobytes() == c_before.tobytes()


# ---- 5. device vectors -------------------------------------------------------------------------------------------------------
def device_vectors(lib, to_device=None, to_host=None, kind="tets2", scheme="mpfa"):
    """loads, states and every output in device memory: the bits of the host-array call.  ``to_device(array) ->
    (address, keepalive)``, ``to_host(keepalive) -> array``; the emulation build takes host addresses."""
    if to_device is None:
        to_device = lambda a: (a.ctypes.data, a)  # noqa: E731
        to_host = lambda a: a  # noqa: E731
    P = setup(lib, kind, scheme)
    g, pr, ad, data, ctx = P["g"], P["pr"], P["ad"], P["data"], P["ctx"]
    obs = np.random.default_rng(4).permutation(g.num_cells)[:7]
    loads = P["loads"][:, :7].copy()
    want, _ = adjoint(P, loads=loads, obs=obs)

    def dev(a):
        return to_device(np.ascontiguousarray(a, dtype=np.float64))

    d_loads, d_states = dev(loads), dev(P["states"])
    names = [m for m in ALL if m != "flux_scale"]
    outs = {m: dev(np.zeros_like(want[m])) for m in names}
    ad._assemble(g, data, pr["acc"], None, pr["src"])
    got, info = ctx.advdiff_adjoint(N, d_loads[0], states=d_states[0], obs_cells=obs, want=ALL, device=True,
                                    out_ptrs={m: outs[m][0] for m in names})
    assert info["steps_done"] == N
    assert got["flux_scale"] == want["flux_scale"]
    for m in names:
        assert np.asarray(to_host(outs[m][1])).ravel().tobytes() == want[m].tobytes(), m


# ---- 6. the fallback path ------------------------------------------------------------------------------------------------
def fallback_path(lib, n=4):
    """The setting of _advdiff_cases.fallback_path: an AMG-preconditioned solve that cannot finish (one iteration
    allowed) is restored from the kept state, handed to Jacobi-GMRES and counted -- one Jacobi-GMRES iteration does not
    get there either, so the call is refused and writes nothing; the next call has the bits of a fresh handle and its
    gradients lie within WHOLE_BOUND."""
    g = UP.tets(n)
    P = setup(lib, None, "mpfa", g=g, pr=AD.problem(g), rtol=1e-12)
    ctx = P["ctx"]
    ref, info = adjoint(P)
    assert info["steps_done"] == N and ctx.stats()["advdiff_adjoint_precond_fallbacks"] == 0
    got, info = adjoint(P, maxit=1, raise_on_fail=False)
    st = ctx.stats()
    assert info["steps_done"] == 0 and not info["converged"]
    assert st["advdiff_adjoint_precond_fallbacks"] == 1 and st["advdiff_adjoint_gmres_retries"] == 0
    assert st["advdiff_adjoint_steps"] == 0
    assert all(np.all(np.asarray(v) == 0.0) for v in got.values())  # no gradient is written
    with pytest.raises(pa.PorefvError) as e:
        adjoint(P, maxit=1)
    assert e.value.status == 6 and e.value.info["steps_done"] == 0
    again, info = adjoint(P)
    assert info["steps_done"] == N and ctx.stats()["advdiff_adjoint_precond_fallbacks"] == 0
    for m in ALL:
        assert np.asarray(again[m]).tobytes() == np.asarray(ref[m]).tobytes(), m
    jref, _ = judged(P)
    err = relative_errors(again, jref, ALL)
    print("after the refused call:", fmt(err))
    assert max(err.values()) <= WHOLE_BOUND


def gmres_retry_path(lib, kind):
    """A BiCGStab step that breaks down is solved again with GMRES from the kept state and counted, and the gradients
    stand.  Pure advection (no conduction: S is the upwind matrix of an acyclic flux, triangular in flow order), one
    observation cell, a load at the last step only, Jacobi, started from lambda^{N+1} = 0: after the first half-step the
    residual is zero in the observation cell, so rho = (r_hat, r) = 0 and the residual turns NaN -- the forward loop's
    injection into a field at rest (_upwind_cases.injection_from_rest), transposed.  The later steps start from a
    lambda^{n+1} that fills the upstream cone and do not break down.  (No conductivity gradient: K = 0.)"""
    g = grid(kind)
    P = setup(lib, None, "tpfa", g=g, pr=AD.problem(g, diffusivity=0.0), precond="jacobi")
    want = tuple(m for m in ALL if m != "conductivity")
    for cell in (0, g.num_cells // 2):
        loads, obs = np.zeros((N, 1)), np.array([cell])
        loads[-1, 0] = 1.3
        got, info = adjoint(P, loads=loads, obs=obs, precond="jacobi", want=want)
        st = P["ctx"].stats()
        with np.errstate(divide="ignore", invalid="ignore"):  # (the judge's t_e of K = 0; its conductivity is not used)
            ref, _ = judged(P, loads=loads, obs=obs)
        err = relative_errors(got, ref, want)
        print(f"GMRES retry on {kind}, observation cell {cell}: {st['advdiff_adjoint_gmres_retries']} retries,", fmt(err))
        assert info["steps_done"] == N and info["converged"]
        assert st["advdiff_adjoint_gmres_retries"] == 1 and st["advdiff_adjoint_precond_fallbacks"] == 0
        assert max(err.values()) <= WHOLE_BOUND


# ---- 7. Mpfa: the conductivity gradient is the two-point product rule -----------------------------------------------------
def mpfa_consistency(lib, kind):
    """For a random direction dK: sum grad_conductivity o dK = sum_f zw_f dt_f, dt_f the directional derivative of the
    two-point transmissibility of the judge's half_faces, zw rebuilt from the library's multipliers."""
    P = setup(lib, kind, "mpfa", w=1.7)
    g, pr = P["g"], P["pr"]
    grads, info = adjoint(P, want=("conductivity", "multipliers"), rtol=1e-13)
    assert info["steps_done"] == N
    _, _, Bsum, U, D = handle_pieces(P)
    _, _, zw = formulas(g, pr["bc"], pr["bv"], P["K"], P["q"], P["w"], pr["acc"], Bsum, U, D, grads["multipliers"],
                        P["states"])
    fi, ci, sg, d, tf, dt = FA.half_faces(g, P["K"])
    dK = np.random.default_rng(9).standard_normal((3, 3, g.num_cells))
    dtf = np.bincount(fi, weights=np.einsum("rse,rse->e", dt, dK[:, :, ci]), minlength=g.num_faces)
    lhs, rhs = np.sum(grads["conductivity"] * dK), zw @ dtf
    scale = np.abs(grads["conductivity"] * dK).sum() + np.abs(zw * dtf).sum()
    print(f"two-point product rule on {kind}: {lhs:.15e} against {rhs:.15e}, {abs(lhs - rhs) / scale:.1e} of the sum of "
          "absolute terms")
    assert scale > 0 and abs(lhs - rhs) <= 1e-13 * scale


# ---- 8. the chain: flow solve -> resident flux -> advection-diffusion -> adjoint -> adjoint_flow --------------------------
def chain(lib, h=1e-4, n_steps=3, w=2.5):
    g = FA.grid("cart6x5")
    rng = np.random.default_rng(21)
    nc, nf = g.num_cells, g.num_faces
    kiso = np.exp(rng.uniform(-0.5, 0.5, nc))
    K = np.zeros((3, 3, nc))
    K[0, 0] = K[1, 1] = K[2, 2] = kiso
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)
    fbv = np.zeros(nf)
    fbv[bf] = 2.0 - g.face_centers[0, bf] - 0.7 * g.face_centers[1, bf]
    fdata = pa.initialize_data({}, "flow", {"second_order_tensor": FA.tensor(K), "bc": bc, "bc_values": fbv})
    flow = pa.Tpfa("flow", library=lib)
    flow.discretize(g, fdata)
    p, info = flow.solve(g, fdata, rtol=1e-13)
    assert info["converged"]
    res = flow.darcy_flux(g, fdata, p, resident=True)
    q = FA.handle(flow, g).resident_flux()
    # the transport: conduction 0.05 x a heterogeneous tensor, Dirichlet on the boundary, flux scale w
    KT = np.zeros((3, 3, nc))
    KT[0, 0] = KT[1, 1] = KT[2, 2] = 0.05 * (1 + rng.random(nc))
    tbv = np.zeros(nf)
    tbv[bf] = rng.random(bf.size)
    acc = 0.3 * g.cell_volumes / 0.4
    c0, src = rng.random(nc), g.cell_volumes * rng.random(nc)
    loads = rng.standard_normal((n_steps, nc))
    par = {"second_order_tensor": FA.tensor(KT), "bc": bc, "bc_values": tbv, "darcy_flux": res, "flux_scale": w}
    tdata = pa.initialize_data({}, KW, par)
    ad = pa.AdvectionDiffusion(KW, scheme="tpfa", library=lib)
    ad.discretize(g, tdata)
    assert ad.context(g) is not FA.handle(flow, g)
    _, ti, states = ad.advance(g, tdata, c0, n_steps, acc, source=src, rtol=1e-13, return_states=True)
    assert ti["steps_done"] == n_steps
    tg, ti = ad.adjoint(g, tdata, n_steps, acc, loads, states, source=src, want=("flux",))
    assert ti["steps_done"] == n_steps
    got, info = flow.adjoint_flow(g, fdata, p, grad_flux=tg["flux"], want=FA.GRADS)
    assert info["converged"]
    # the judge's scipy chain on the exported matrices
    md = tdata[pa.DISCRETIZATION_MATRICES][KW]
    _, A, Bsum, U, D = pieces(g, bc, q, w, md["flux"], md["bound_flux"])
    cf = sps.csr_matrix(g.cell_faces)
    S = sps.csr_matrix(sps.diags(acc) + A)
    b = -(cf.T @ (Bsum @ tbv))

    def transport(S_, b_):
        solve = refined(sps.csc_matrix(S_))
        st = np.empty((n_steps + 1, nc))
        st[0] = c0
        for k in range(n_steps):
            st[k + 1] = solve(acc * st[k] + b_ + src)
        return st

    jstates = transport(S, b)
    lam = multipliers(S, acc, loads)
    jt, _, _ = formulas(g, bc, tbv, KT, q, w, acc, Bsum, U, D, lam, jstates)
    P = dict(g=g, K=K, bc=bc, bv=fbv, vs=None, p=p, flow=flow, gq=jt["flux"], gp=None)
    ref = FA.judged(P, "flux")
    err = FA.relative_errors(got, ref, FA.GRADS)
    print("the chain against the judge's scipy chain:", fmt(err))
    assert max(err.values()) <= WHOLE_BOUND
    # central differences of the judge's whole forward chain (numpy alone), valid while no face changes its upstream side
    TD, BD, _ = FA.tpfa_numpy(g, KT, bc)

    def run(K_):
        _, q_ = FA.forward_numpy(g, K_, bc, fbv, np.zeros(nc), None)
        _, A_, Bs_, _, _ = pieces(g, bc, q_, w, TD, BD)
        st = transport(sps.csr_matrix(sps.diags(acc) + A_), -(cf.T @ (Bs_ @ tbv)))
        return float(np.sum(loads * st[1:])), q_

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


# ---- 9. return_states ----------------------------------------------------------------------------------------------------
def return_states(lib, kind="tets2", scheme="mpfa"):
    g = grid(kind)
    pr = AD.problem(g)
    ad, data = AD.discretized(lib, g, pr, scheme)
    c, info, states = ad.advance(g, data, pr["c0"], N, pr["acc"], source=pr["src"], return_states=True)
    assert info["steps_done"] == N and info["converged"] and states.shape == (N + 1, g.num_cells)
    assert states[0].tobytes() == np.asarray(pr["c0"], dtype=float).tobytes() and states[N].tobytes() == c.tobytes()
    one = pr["c0"]
    for k in range(N):
        one, i1 = ad.advance(g, data, one, 1, pr["acc"], source=pr["src"])
        assert i1["steps_done"] == 1 and one.tobytes() == states[k + 1].tobytes(), k
    run, info = ad.advance(g, data, pr["c0"], N, pr["acc"], source=pr["src"])
    assert len((run, info)) == 2 and run.tobytes() == states[N].tobytes()


# ---- 10. refusals ------------------------------------------------------------------------------------------------------------
def _raw(ctx, loads, states, want, method=None, n_steps=N):
    """pfv_advdiff_adjoint itself, the outputs pre-filled with 7.5: (status, outputs)"""
    dp = _lib._dp
    shapes = {"c0": ctx.nc, "source": ctx.nc, "bc_values": ctx.nf, "accumulation": ctx.nc, "flux": ctx.nf, "flux_scale": 1,
              "conductivity": 9 * ctx.nc, "multipliers": n_steps * ctx.nc}
    outs = {m: np.full(shapes[m], 7.5) for m in want}
    ptr = lambda m: _lib._ptr(outs.get(m), dp)  # noqa: E731
    done, info = C.c_int32(0), _lib.SolveInfo()
    st = ctx.lib.pfv_advdiff_adjoint(ctx._h, n_steps, ctx.nc, None, _lib._ptr(loads, dp), _lib._ptr(states, dp),
                                     _lib.SOLVE_BICGSTAB if method is None else method, 1e-12, 1000, ptr("c0"),
                                     ptr("source"), ptr("bc_values"), ptr("accumulation"), ptr("flux"), ptr("flux_scale"),
                                     ptr("conductivity"), ptr("multipliers"), C.byref(done), C.byref(info))
    return st, outs


def refusals(lib):
    P = setup(lib, "tets2", "mpfa")
    g, pr, ad, data, ctx = P["g"], P["pr"], P["ad"], P["data"], P["ctx"]
    nc = g.num_cells
    c_ref, _ = ad.advance(g, data, pr["c0"], N, pr["acc"], source=pr["src"])
    loads, states = np.ascontiguousarray(P["loads"]), np.ascontiguousarray(P["states"])
    # ---- status 4.  No active advection-diffusion system: after a flow assembly, after an adjoint call
    ad.assemble_matrix_rhs(g, data)
    ad.diffusion.assemble_matrix_rhs(g, data)
    with pytest.raises(pa.PorefvError, match="pfv_advdiff_assemble first") as e:
        ctx.advdiff_adjoint(N, loads)
    assert e.value.status == 4
    adjoint(P)
    with pytest.raises(pa.PorefvError, match="pfv_advdiff_assemble first") as e:
        ctx.advdiff_adjoint(N, loads)
    assert e.value.status == 4
    # another method
    with pytest.raises(ValueError, match="PFV_SOLVE_BICGSTAB or PFV_SOLVE_GMRES"):
        adjoint(P, method="cg")
    # obs_cells out of range, repeated
    with pytest.raises(ValueError, match=rf"obs_cells\[1\] = {nc} is out of range"):
        adjoint(P, loads=loads[:, :3], obs=np.array([0, nc, 2]))
    with pytest.raises(ValueError, match=r"obs_cells\[2\] = 5 is repeated"):
        adjoint(P, loads=loads[:, :3], obs=np.array([5, 1, 5]))
    # a non-finite load: the lowest index is named
    bad = loads.copy()
    bad[2, 9] = np.nan
    bad[1, [17, 4]] = np.inf
    with pytest.raises(ValueError, match="loads is not finite at step 2, component 0, observation 4"):
        adjoint(P, loads=bad)
    # the four gradients that need states: refused by the class and by the call itself, which writes nothing
    for m in ("accumulation", "flux", "flux_scale", "conductivity"):
        with pytest.raises(ValueError, match="needs states"):
            adjoint(P, want=(m,), states=None)
        ad._assemble(g, data, pr["acc"], None, pr["src"])
        st, outs = _raw(ctx, loads, None, (m, "source"))
        assert st == 4 and f"grad_{m} needs states" in ctx.lib.pfv_last_error(ctx._h).decode()
        assert all(np.all(a == 7.5) for a in outs.values())
    # ---- status 6: a step that does not converge writes no gradient
    ad._assemble(g, data, pr["acc"], None, pr["src"])
    ctx._select_precond("jacobi")
    dp = _lib._dp
    marks = {m: np.full(n, 7.5) for m, n in (("c0", nc), ("multipliers", N * nc), ("flux", g.num_faces))}
    done, info = C.c_int32(0), _lib.SolveInfo()
    st = ctx.lib.pfv_advdiff_adjoint(ctx._h, N, nc, None, _lib._ptr(loads, dp), _lib._ptr(states, dp), _lib.SOLVE_BICGSTAB,
                                     1e-12, 1, _lib._ptr(marks["c0"], dp), None, None, None, _lib._ptr(marks["flux"], dp),
                                     None, None, _lib._ptr(marks["multipliers"], dp), C.byref(done), C.byref(info))
    assert st == 6 and done.value == 0 and info.converged == 0
    assert all(np.all(a == 7.5) for a in marks.values())
    with pytest.raises(RuntimeError, match="no assembled system"):
        ctx.solve()  # (no active system after a refused step either)
    # ---- status 5.  PFV_PRECOND_SWEEP
    with pytest.raises(pa.PorefvError, match="later pull request") as e:
        adjoint(P, precond="sweep")
    assert e.value.status == 5 and "PFV_PRECOND_SWEEP" in e.value.message
    # after the refusals: assemble + advance as before
    c_now, info = ad.advance(g, data, pr["c0"], N, pr["acc"], source=pr["src"])
    assert info["steps_done"] == N and c_now.tobytes() == c_ref.tobytes()
    # a Robin face (refused by the assembly already), an internal-boundary face: the first one is named
    bf = g.get_all_boundary_faces()
    interior = np.flatnonzero(~np.isin(np.arange(g.num_faces), bf))
    labels = list(np.array(["dir", "neu", "dir"])[np.arange(bf.size) % 3])
    labels[4] = labels[9] = "rob"
    for scheme in ("mpfa", "tpfa"):
        pr_r = AD.problem(g)
        pr_r["par"]["bc"] = pa.BoundaryCondition(g, bf, labels)
        ad_r, data_r = AD.discretized(lib, g, pr_r, scheme)
        with pytest.raises(pa.PorefvError, match=f"face {bf[4]} ") as e:
            ad_r.adjoint(g, data_r, N, pr["acc"], loads, states)
        assert e.value.status == 5 and "Robin" in e.value.message
        pr_i = AD.problem(g)
        inner = pa.BoundaryCondition(g, bf, list(np.array(["dir", "neu", "dir"])[np.arange(bf.size) % 3]))
        inner.is_internal[[interior[6], interior[3]]] = True
        pr_i["par"]["bc"] = inner
        ad_i, data_i = AD.discretized(lib, g, pr_i, scheme)
        with pytest.raises(pa.PorefvError, match=f"face {interior[3]} ") as e:
            ad_i.adjoint(g, data_i, N, pr["acc"], loads, states)
        assert e.value.status == 5 and "INTERNAL" in e.value.message
    # a partial discretization: the rows of the other faces are zero
    pr_p = AD.problem(g)
    pr_p["par"]["specified_cells"] = np.array([0, 1])
    ad_p, data_p = AD.discretized(lib, g, pr_p, "mpfa")
    with pytest.raises(pa.PorefvError) as e:
        ad_p.adjoint(g, data_p, N, pr["acc"], loads, states)
    assert e.value.status == 5 and "partial" in e.value.message
    # a periodic grid: what the forward class refuses
    gp = UP.geo(pa.CartGrid([3, 3], [1.0, 1.0]))
    gp.periodic_face_map = np.vstack([np.flatnonzero(np.isclose(gp.face_centers[0], 0.0)),
                                      np.flatnonzero(np.isclose(gp.face_centers[0], 1.0))])
    with pytest.raises(pa.PorefvError) as e:
        pa.AdvectionDiffusion(KW, library=lib).adjoint(gp, pa.initialize_data({}, KW, AD.problem(gp)["par"]), N,
                                                       np.ones(gp.num_cells), np.zeros((N, gp.num_cells)), None)
    assert e.value.status == 5 and "periodic" in e.value.message


# ---- 11. the handle after the call ------------------------------------------------------------------------------------------
def handle_afterwards(lib, kind="tets2"):
    """Flow and transport on ONE handle: after the adjoint pfv_solve asks for an assembly; the flow order, the resident
    flux and the flux matrix are as they were."""
    g = grid(kind)
    pr = AD.problem(g)
    data = pa.initialize_data({}, KW, dict(pr["par"]))
    mp = pa.Mpfa(KW, library=lib)
    mp.discretize(g, data)
    p, _ = mp.solve(g, data, rtol=1e-13)
    mp.darcy_flux(g, data, p, resident=True)
    ad = pa.AdvectionDiffusion(KW, diffusion=mp, library=lib)
    ctx = ad.context(g)
    assert ctx is mp.context(g)
    _, info, states = ad.advance(g, data, pr["c0"], N, pr["acc"], source=pr["src"], precond="sweep", return_states=True)
    assert info["steps_done"] == N
    order, q_res = ctx.sweep_info(), ctx.resident_flux()
    flux = sps.csr_matrix(ctx.matrix(_lib.MAT_FLUX))
    loads = np.random.default_rng(2).standard_normal((N, g.num_cells))
    grads, info = ad.adjoint(g, data, N, pr["acc"], loads, states, source=pr["src"], want=ALL)
    assert info["steps_done"] == N
    with pytest.raises(RuntimeError, match="no assembled system"):
        ctx.solve()
    with pytest.raises(pa.PorefvError, match="pfv_advdiff_assemble first") as e:
        ctx.advdiff_advance(pr["c0"], 1)
    assert e.value.status == 4
    after = ctx.sweep_info()
    assert sorted(after) == sorted(order)
    for k in order:
        assert np.asarray(after[k]).tobytes() == np.asarray(order[k]).tobytes(), k
    assert ctx.resident_flux().tobytes() == q_res.tobytes()
    UP.same_csr(sps.csr_matrix(ctx.matrix(_lib.MAT_FLUX)), flux, "flux after the adjoint")
    c_again, info = ad.advance(g, data, pr["c0"], N, pr["acc"], source=pr["src"], precond="sweep")
    assert info["steps_done"] == N and c_again.tobytes() == states[N].tobytes()
