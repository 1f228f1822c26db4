"""Cases of the exact conductivity gradient of the advection-diffusion adjoint (``want="conductivity_exact"`` of
``AdvectionDiffusion.adjoint`` / ``Context.advdiff_adjoint``, pfv_advdiff_adjoint_exact), shared by the emulation suite
(test_advdiff_exact_emulation.py) and the GPU suite (test_gpu_advdiff_exact.py): each takes the library to run on.
Grids: CartGrid([6, 5]) of _flow_adjoint_cases, tets(2), tets(3) and the line of _advdiff_adjoint_cases; problems,
N = 4 steps, loads and multipliers are those of _advdiff_adjoint_cases.

The judge (``judge``) is numpy and never calls the new code:

    sum_{n=1..N} exact_formulas(g, K, bc, c^n, bv, None, -(cell_faces lambda^n))      (_mpfa_adjoint_cases.exact_formulas)

and, per entry, the sum of the scales that function returns.

Figures measured with these inputs, on the emulation build and on an MI355X:

- ``judge_against_differences`` (central differences of J = sum_n <g^n, c^n> through N forward steps built from
  oracle.mpfa_oracle.discretize, the numpy upwind of _upwind_cases and a sparse LU; h = 1e-4, every entry of K perturbed
  on its own): tets(3), all nine entries of every seventh cell: worst deviation 7.9e-10 of the largest gradient entry;
  CartGrid([6, 5]), the four in-plane entries of every cell: 1.4e-9.  EXACT_DIFF_BOUND is ten times the larger, 1.4e-8
  (below the 1e-7 above which the formula, not the step size, would be wrong).  The sign of z is settled here.
- ``library_against_judge`` at the library's own multipliers and states, per entry relative to the sum of the absolute
  values of the terms added up, every MPFA grid in both regimes: worst 1.5e-14 on the emulation build (tets(3),
  diffusive; 9.2e-16 of the largest entry), 1.3e-14 on the MI355X (tets(3), diffusive; 1.3e-15 of the largest entry);
  CartGrid([6, 5]) 1.7e-15 / 1.4e-15.  EXACT_SPLIT_BOUND is ten times the emulation value: the order of
  _mpfa_adjoint_cases.EXACT_SPLIT_BOUND, a decade below it (no vector source here).
- ``whole_call`` at the defaults (BiCGStab, AMG, rtol = 1e-12) against the judge on its own LU multipliers, max-norm
  relative error: worst 4.4e-13 on the emulation build and on the MI355X (tets(3), diffusive).
  EXACT_WHOLE_BOUND is ten times the emulation value, far below the 1e-8 above which a formula or the solve would be
  wrong.
- ``library_against_own_differences`` on tets(2), all nine entries of every eleventh cell, through the library's own
  discretize + advance: 7.3e-10 (emulation), 4.6e-10 (MI355X) of the largest entry; bound EXACT_DIFF_BOUND.
- ``it_matters`` on tets(3): "conductivity_exact" and "conductivity" differ by 0.85 of the largest entry on both
  builds (required: more than 100 EXACT_DIFF_BOUND = 1.4e-6).
- ``k_orthogonal``: diagonal entries against a TPFA handle's "conductivity" 2.4e-15 (emulation), 1.5e-15 (MI355X) of
  the sum of the absolute terms."""
import ctypes as C
import functools
import math

import numpy as np
import pytest
import scipy.sparse as sps

import porepy_amd as pa
from oracle import mpfa_oracle as mo
from porepy_amd import _lib
from tests import _advdiff_adjoint_cases as AA
from tests import _advdiff_cases as AD
from tests import _flow_adjoint_cases as FA
from tests import _mpfa_adjoint_cases as MA
from tests import _upwind_cases as UP
from tests._advdiff_adjoint_cases import ALL, N
from tests._advdiff_cases import KW
from tests._react_adjoint_cases import refined

KEY = "conductivity_exact"
EXACT_DIFF_BOUND = 10 * 1.4e-9     # ten times the worst value judge_against_differences reports
EXACT_SPLIT_BOUND = 10 * 1.5e-14   # ten times the worst emulation value of library_against_judge
EXACT_WHOLE_BOUND = 10 * 4.4e-13   # ten times the worst emulation value of whole_call
MPFA_GRIDS = ("cart6x5", "tets2", "tets3")
DEFAULT_BATCH = 32  # include/porefv.h: exact_batch = 0
ALL_ENTRIES = MA.ALL_ENTRIES
PLANE_ENTRIES = ((0, 0), (0, 1), (1, 0), (1, 1))


@functools.lru_cache(maxsize=None)
def grid(kind):
    return FA.grid(kind) if kind == "cart6x5" else AA.grid(kind)


def setup(lib, kind, scheme="mpfa", regime="diffusive", **kw):
    return AA.setup(lib, kind, scheme, regime, g=grid(kind), **kw)


# ---- the judge --------------------------------------------------------------------------------------------------------
def judge(g, K, bc, bv, lam, states):
    """(grad, scale): the exact conductivity gradient at given multipliers lambda^1 .. lambda^N and states c^0 .. c^N"""
    cf = sps.csr_matrix(g.cell_faces)
    grad, scale = np.zeros((3, 3, g.num_cells)), np.zeros((3, 3, g.num_cells))
    for k in range(lam.shape[0]):
        gk, sk = MA.exact_formulas(g, K, bc, states[k + 1], bv, None, -(cf @ lam[k]))
        grad += gk
        scale += sk
    return grad, scale


def judge_of(P, lam, states=None):
    pr = P["pr"]
    return judge(P["g"], P["K"], pr["bc"], pr["bv"], lam, P["states"] if states is None else states)


def own_multipliers(P):
    """the judge's own lambda: a sparse LU with one step of refinement on the handle's matrices"""
    S, _, _, _, _ = AA.handle_pieces(P)
    return AA.multipliers(S, P["pr"]["acc"], P["loads"])


def scaled_error(got, ref, scale):
    return AA.scaled_errors({KEY: got}, {KEY: ref}, {KEY: scale}, (KEY,))[KEY]


# ---- 1. the judge against central differences (no library) ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def difference_problem(kind):
    """The problem of ``judge_against_differences`` and the judge's gradient at it: computed once per grid, shared by the
    cases that difference one entry of K each, and left unchanged."""
    g = grid(kind)
    pr = AD.problem(g)
    bc, bv, acc, nc = pr["bc"], pr["bv"], pr["acc"], g.num_cells
    K = np.array(pr["par"]["second_order_tensor"].values, dtype=float)
    q, w = np.asarray(pr["q"], dtype=float), 1.7
    loads = np.random.default_rng(31).standard_normal((N, nc))
    raw, bcraw = pa.grid_to_raw(g), pa.bc_to_raw(bc)

    def run(K_):
        mats = mo.discretize(raw, K_, bcraw)
        cf, A, Bsum, _, _ = AA.pieces(g, bc, q, w, mats["flux"], mats["bound_flux"])
        S = sps.csr_matrix(sps.diags(acc) + A)
        b = -(cf.T @ (Bsum @ bv))
        solve = refined(sps.csc_matrix(S))
        states = np.empty((N + 1, nc))
        states[0] = pr["c0"]
        for k in range(N):
            states[k + 1] = solve(acc * states[k] + b + pr["src"])
        return float(np.sum(loads * states[1:])), S, states

    _, S, states = run(K)
    gk, _ = judge(g, K, bc, bv, AA.multipliers(S, acc, loads), states)
    gk.setflags(write=False)
    K.setflags(write=False)
    return g, K, (lambda K_: run(K_)[0]), gk


def judge_against_differences(kind="tets3", h=1e-4, stride=7, entries=ALL_ENTRIES):
    g, K, J, gk = difference_problem(kind)
    worst = 0.0
    for c in range(0, g.num_cells, stride):
        for r, s in entries:
            Kp, Km = K.copy(), K.copy()
            Kp[r, s, c] += h
            Km[r, s, c] -= h
            worst = max(worst, abs((J(Kp) - J(Km)) / (2 * h) - gk[r, s, c]) / np.abs(gk).max())
    print(f"exact conductivity judge against central differences on {kind} (h = {h:g}), entries {list(entries)}: "
          f"{worst:.1e} of the largest entry")
    if g.dim == 2:
        assert np.all(gk[2] == 0.0) and np.all(gk[:, 2] == 0.0)
    assert EXACT_DIFF_BOUND <= 1e-7 and worst <= EXACT_DIFF_BOUND
    return worst


# ---- 2. the library against the judge, at the library's own multipliers ------------------------------------------------
def library_against_judge(lib, kind, regime):
    P = setup(lib, kind, "mpfa", regime, w=1.7)
    grads, info = AA.adjoint(P, want=("multipliers", KEY), rtol=1e-13, precond="jacobi")
    assert info["steps_done"] == N and grads[KEY].shape == (3, 3, P["g"].num_cells)
    ref, scale = judge_of(P, grads["multipliers"])
    err = scaled_error(grads[KEY], ref, scale)
    print(f"exact conductivity gradient against the judge, mpfa on {kind}, {regime}: {err:.1e} of the sum of absolute "
          f"terms, {np.abs(grads[KEY] - ref).max() / np.abs(ref).max():.1e} of the largest entry")
    if P["g"].dim == 2:  # only the 2 x 2 block
        assert np.all(grads[KEY][2] == 0.0) and np.all(grads[KEY][:, 2] == 0.0)
    assert np.abs(ref).max() > 0.0 and err <= EXACT_SPLIT_BOUND
    return err


# ---- 3. the whole call at the defaults against the judge's own multipliers -----------------------------------------------
def whole_call(lib, kind, regime):
    P = setup(lib, kind, "mpfa", regime, w=1.7, rtol=1e-12)
    grads, info = AA.adjoint(P, want=(KEY,))  # the defaults: BiCGStab, AMG, rtol = 1e-12
    ref, _ = judge_of(P, own_multipliers(P))
    err = float(np.abs(grads[KEY] - ref).max() / np.abs(ref).max())
    print(f"whole call, mpfa on {kind}, {regime}: max-norm relative error {err:.1e}")
    assert info["steps_done"] == N and info["converged"] and sorted(grads) == [KEY]
    assert EXACT_WHOLE_BOUND <= 1e-8 and err <= EXACT_WHOLE_BOUND
    return err


# ---- 4. end to end: the library against central differences of its own forward run --------------------------------------
def library_against_own_differences(lib, kind="tets2", h=1e-4, stride=11):
    P = setup(lib, kind, "mpfa", rtol=1e-13, precond="jacobi")
    g, pr = P["g"], P["pr"]
    got, info = AA.adjoint(P, want=(KEY,), rtol=1e-13, precond="jacobi")
    assert info["steps_done"] == N

    def J(K_):
        pr_ = dict(pr, par=dict(pr["par"], second_order_tensor=FA.tensor(K_)))
        ad, data = AD.discretized(lib, g, pr_, "mpfa")
        _, i, states = ad.advance(g, data, pr["c0"], N, pr["acc"], source=pr["src"], rtol=1e-13, precond="jacobi",
                                  return_states=True)
        assert i["steps_done"] == N
        return float(np.sum(P["loads"] * states[1:]))

    worst = 0.0
    for c in range(0, g.num_cells, stride):
        for r, s in ALL_ENTRIES:
            Kp, Km = P["K"].copy(), P["K"].copy()
            Kp[r, s, c] += h
            Km[r, s, c] -= h
            worst = max(worst, abs((J(Kp) - J(Km)) / (2 * h) - got[KEY][r, s, c]) / np.abs(got[KEY]).max())
    print(f"exact conductivity gradient against central differences of the library's own run on {kind} (h = {h:g}): "
          f"{worst:.1e} of the largest entry")
    assert worst <= EXACT_DIFF_BOUND
    return worst


# ---- 5. it matters -------------------------------------------------------------------------------------------------------
def it_matters(lib):
    P = setup(lib, "tets3", "mpfa")
    grads, info = AA.adjoint(P, want=("conductivity", KEY))
    assert info["steps_done"] == N
    diff = np.abs(grads[KEY] - grads["conductivity"]).max() / np.abs(grads[KEY]).max()
    print(f"tets3: exact conductivity gradient against the two-point rule, {diff:.2e} of the largest entry")
    assert diff > 100 * EXACT_DIFF_BOUND
    return diff


# ---- 6. the batch size changes no bit ----------------------------------------------------------------------------------
def batch_invariance(lib, kind="tets2"):
    P = setup(lib, kind, "mpfa")
    g, pr, ad, ctx = P["g"], P["pr"], P["ad"], P["ctx"]
    kw = dict(want=(KEY,), rtol=1e-13, precond="jacobi")
    ref, _ = AA.adjoint(P, exact_batch=N, **kw)
    st = ctx.stats()
    classes = st["advdiff_adjoint_exact_passes"]  # B = N: one batch, one launch per non-empty node class
    assert classes >= 1 and st["advdiff_adjoint_exact_batch"] == N and st["advdiff_adjoint_exact_ms"] >= 0.0
    assert np.abs(ref[KEY]).max() > 0.0
    for batch in (1, 3, 4, 5, 0, 3):
        got, info = AA.adjoint(P, exact_batch=batch, **kw)
        st = ctx.stats()
        used = min(batch if batch else DEFAULT_BATCH, N)
        assert info["steps_done"] == N and got[KEY].tobytes() == ref[KEY].tobytes(), batch
        assert st["advdiff_adjoint_exact_batch"] == used, batch
        assert st["advdiff_adjoint_exact_passes"] == math.ceil(N / used) * classes, batch
    dflt, _ = AA.adjoint(P, **kw)  # (exact_batch not given)
    assert dflt[KEY].tobytes() == ref[KEY].tobytes()
    # N = 1: one state, whatever B; N = 0: zeros, no pass
    one = {}
    for batch in (0, 1, 3):
        one[batch], info = ad.adjoint(g, P["data"], 1, pr["acc"], P["loads"][:1], P["states"][:2], source=pr["src"],
                                      exact_batch=batch, **kw)
        st = ctx.stats()
        assert info["steps_done"] == 1 and one[batch][KEY].tobytes() == one[0][KEY].tobytes()
        assert st["advdiff_adjoint_exact_batch"] == 1 and st["advdiff_adjoint_exact_passes"] == classes
    lam = ad.adjoint(g, P["data"], 1, pr["acc"], P["loads"][:1], P["states"][:2], source=pr["src"], want=("multipliers",),
                     rtol=1e-13, precond="jacobi")[0]["multipliers"]
    r1, s1 = judge_of(P, lam, P["states"][:2])
    assert scaled_error(one[0][KEY], r1, s1) <= EXACT_SPLIT_BOUND
    none, info = ad.adjoint(g, P["data"], 0, pr["acc"], P["loads"][:0], P["states"][:1], source=pr["src"], **kw)
    st = ctx.stats()
    assert info["steps_done"] == 0 and none[KEY].shape == (3, 3, g.num_cells) and np.all(none[KEY] == 0.0)
    assert st["advdiff_adjoint_exact_passes"] == 0
    # a call without the key: no pass, the statistics say so
    AA.adjoint(P, want=("conductivity",))
    st = ctx.stats()
    assert st["advdiff_adjoint_exact_passes"] == 0 and st["advdiff_adjoint_exact_batch"] == 0
    assert st["advdiff_adjoint_exact_ms"] == 0.0


# ---- 7. the other outputs keep their bits; the handle afterwards ---------------------------------------------------------
def other_outputs_unchanged(lib, kind="tets2"):
    """Flow and transport on ONE handle, as in _advdiff_adjoint_cases.handle_afterwards."""
    g = grid(kind)
    pr = AD.problem(g)
    data = pa.initialize_data({}, KW, dict(pr["par"]))
    mp = pa.Mpfa(KW, library=lib)
    mp.discretize(g, data)
    p, _ = mp.solve(g, data, rtol=1e-13)
    mp.darcy_flux(g, data, p, resident=True)
    ad = pa.AdvectionDiffusion(KW, diffusion=mp, library=lib)
    ctx = ad.context(g)
    _, info, states = ad.advance(g, data, pr["c0"], N, pr["acc"], source=pr["src"], precond="sweep", return_states=True)
    assert info["steps_done"] == N
    order, q_res = ctx.sweep_info(), ctx.resident_flux()
    flux = sps.csr_matrix(ctx.matrix(_lib.MAT_FLUX))
    loads = np.random.default_rng(2).standard_normal((N, g.num_cells))
    plain, info = ad.adjoint(g, data, N, pr["acc"], loads, states, source=pr["src"], want=ALL)
    assert info["steps_done"] == N
    for batch in (None, 1, 3):
        both, info = ad.adjoint(g, data, N, pr["acc"], loads, states, source=pr["src"], want=ALL + (KEY,),
                                exact_batch=batch)
        assert info["steps_done"] == N and sorted(both) == sorted(ALL + (KEY,))
        for m in ALL:
            assert np.asarray(both[m]).tobytes() == np.asarray(plain[m]).tobytes(), (batch, m)
    only, _ = ad.adjoint(g, data, N, pr["acc"], loads, states, source=pr["src"], want=(KEY,))
    assert only[KEY].tobytes() == both[KEY].tobytes()
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


# ---- 8. a K-orthogonal grid: the exact MPFA gradient is the two-point one ------------------------------------------------
def k_orthogonal(lib):
    g = UP.geo(pa.CartGrid([6, 5]))
    pr = AD.problem(g)
    nc = g.num_cells
    K = np.zeros((3, 3, nc))
    for r in range(3):
        K[r, r] = np.exp(np.random.default_rng(31 + r).uniform(-1.0, 1.0, nc))
    pr["par"]["second_order_tensor"] = FA.tensor(K)
    P = AA.setup(lib, None, "mpfa", g=g, pr=pr, w=1.7)
    kw = dict(rtol=1e-13, precond="jacobi")
    exact, info = AA.adjoint(P, want=("multipliers", KEY), **kw)
    assert info["steps_done"] == N
    ad_t, data_t = AD.discretized(lib, g, pr, "tpfa")
    two, info = ad_t.adjoint(g, data_t, N, pr["acc"], P["loads"], P["states"], source=pr["src"], want=("conductivity",), **kw)
    assert info["steps_done"] == N
    _, scale = judge_of(P, exact["multipliers"])
    worst = 0.0
    for r in range(g.dim):
        diff, sc = np.abs(exact[KEY][r, r] - two["conductivity"][r, r]), scale[r, r]
        assert np.all(diff[sc == 0.0] == 0.0)
        worst = max(worst, float((diff[sc > 0] / sc[sc > 0]).max()))
    print(f"K-orthogonal grid: diagonal entries of the exact MPFA gradient against the TPFA gradient, {worst:.1e} of the "
          "sum of absolute terms")
    assert worst <= EXACT_SPLIT_BOUND


# ---- 9. TPFA and the 1-D delegate -----------------------------------------------------------------------------------------
def tpfa_and_delegate(lib):
    for kind, scheme in (("tets2", "tpfa"), ("line", "mpfa"), ("line", "tpfa")):
        P = setup(lib, kind, scheme)
        got, info = AA.adjoint(P, want=("conductivity", KEY))
        assert info["steps_done"] == N and got[KEY].tobytes() == got["conductivity"].tobytes(), (kind, scheme)
        assert np.abs(got[KEY]).max() > 0.0 and got[KEY].shape == (3, 3, P["g"].num_cells)
        only, _ = AA.adjoint(P, want=(KEY,))
        assert sorted(only) == [KEY] and only[KEY].tobytes() == got[KEY].tobytes(), (kind, scheme)
        assert P["ctx"].stats()["advdiff_adjoint_exact_passes"] == 0  # (no region pass)


# ---- 10. device vectors ---------------------------------------------------------------------------------------------------
def device_vectors(lib, to_device=None, to_host=None, kind="tets2"):
    """loads, states and every output in device memory: the bits of the host-array call, for every batch size (the
    states are read in place, backwards)."""
    if to_device is None:
        to_device = lambda a: (a.ctypes.data, a)  # noqa: E731
        to_host = lambda a: a  # noqa: E731
    P = setup(lib, kind, "mpfa")
    g, pr, ad, data, ctx = P["g"], P["pr"], P["ad"], P["data"], P["ctx"]
    names = ("accumulation", "conductivity", KEY)
    want, _ = AA.adjoint(P, want=names)
    plain, _ = AA.adjoint(P, want=(KEY,))  # (host states staged straight into the ring)
    assert plain[KEY].tobytes() == want[KEY].tobytes()

    def dev(a):
        return to_device(np.ascontiguousarray(a, dtype=np.float64))

    d_loads, d_states = dev(P["loads"]), dev(P["states"])
    for batch in (0, 1, 3):
        outs = {m: dev(np.zeros_like(want[m])) for m in names}
        ad._assemble(g, data, pr["acc"], None, pr["src"])
        _, info = ctx.advdiff_adjoint(N, d_loads[0], states=d_states[0], want=names, device=True,
                                      out_ptrs={m: outs[m][0] for m in names}, exact_batch=batch)
        assert info["steps_done"] == N
        for m in names:
            assert np.asarray(to_host(outs[m][1])).ravel().tobytes() == want[m].tobytes(), (batch, m)


# ---- 11. refusals ---------------------------------------------------------------------------------------------------------
SHAPES = {"c0": "nc", "source": "nc", "bc_values": "nf", "accumulation": "nc", "flux": "nf", "flux_scale": 1,
          "conductivity": "9nc", "multipliers": "Nnc", KEY: "9nc"}


def raw(ctx, loads, states, want, exact=True, method=None, maxit=1000, batch=0, n_steps=N):
    """pfv_advdiff_adjoint_exact (``exact`` False: pfv_advdiff_adjoint) itself, the outputs pre-filled with 7.5:
    (status, message, steps_done, every mark still in place)"""
    dp = _lib._dp
    size = {"nc": ctx.nc, "nf": ctx.nf, 1: 1, "9nc": 9 * ctx.nc, "Nnc": max(n_steps, 1) * ctx.nc}
    outs = {m: np.full(size[SHAPES[m]], 7.5) for m in want}
    ptr = lambda m: _lib._ptr(outs.get(m), dp)  # noqa: E731
    done, info = C.c_int32(0), _lib.SolveInfo()
    args = (ctx._h, n_steps, ctx.nc, None, _lib._ptr(loads, dp), _lib._ptr(states, dp),
            _lib.SOLVE_BICGSTAB if method is None else method, 1e-12, maxit, ptr("c0"), ptr("source"), ptr("bc_values"),
            ptr("accumulation"), ptr("flux"), ptr("flux_scale"), ptr("conductivity"), ptr("multipliers"), C.byref(done),
            C.byref(info))
    st = ctx.lib.pfv_advdiff_adjoint_exact(*args, ptr(KEY), batch) if exact else ctx.lib.pfv_advdiff_adjoint(*args)
    msg = ctx.lib.pfv_last_error(ctx._h).decode() if st else ""
    return st, msg, done.value, all(np.all(a == 7.5) for a in outs.values())


def same_refusal(ctx, prepare, loads, states, want, status, word, **kw):
    """The refusal of pfv_advdiff_adjoint, and the same status and text from the new export, nothing written."""
    prepare()
    old = raw(ctx, loads, states, tuple(m for m in want if m != KEY), exact=False, **kw)
    prepare()
    new = raw(ctx, loads, states, want, **kw)
    assert old[0] == status and word in old[1] and old[3], old
    assert new == old, (old, new)


def refusals(lib):
    P = setup(lib, "tets2", "mpfa")
    g, pr, ad, data, ctx = P["g"], P["pr"], P["ad"], P["data"], P["ctx"]
    nc = g.num_cells
    loads, states = np.ascontiguousarray(P["loads"]), np.ascontiguousarray(P["states"])
    assemble = lambda: ad._assemble(g, data, pr["acc"], None, pr["src"])  # noqa: E731
    # ---- the new ones.  No states: the class, the context and the call itself
    with pytest.raises(ValueError, match="needs states"):
        AA.adjoint(P, want=(KEY,), states=None)
    assemble()
    st, msg, done, untouched = raw(ctx, loads, None, (KEY, "source"))
    assert (st, done, untouched) == (4, 0, True) and "grad_conductivity_exact needs states" in msg
    # a negative batch
    with pytest.raises(ValueError, match="exact_batch must not be negative"):
        AA.adjoint(P, want=(KEY,), exact_batch=-1)
    assemble()
    st, msg, done, untouched = raw(ctx, loads, states, (KEY, "c0"), batch=-1)
    assert (st, done, untouched) == (4, 0, True) and "exact_batch" in msg
    # the unknown key stays unknown, and the message names the new one
    with pytest.raises(ValueError, match="unknown gradient.*conductivity_exact"):
        AA.adjoint(P, want=("conductivity_inexact",))
    assert _lib.Context.ADVDIFF_ADJOINT_EXACT == (KEY,) and KEY not in _lib.Context.ADVDIFF_ADJOINT_GRADIENTS
    # ---- every refusal of pfv_advdiff_adjoint holds for the new export: the same status, the same text, nothing written
    every = ALL + (KEY,)

    def flow_assembly():
        ad.assemble_matrix_rhs(g, data)
        ad.diffusion.assemble_matrix_rhs(g, data)

    same_refusal(ctx, flow_assembly, loads, states, every, 4, "pfv_advdiff_assemble first")
    same_refusal(ctx, assemble, loads, states, every, 4, "PFV_SOLVE_BICGSTAB or PFV_SOLVE_GMRES", method=_lib.SOLVE_CG)
    same_refusal(ctx, assemble, loads, states, every, 4, "n_steps must not be negative", n_steps=-1)
    bad = loads.copy()
    bad[2, 9] = np.nan
    same_refusal(ctx, assemble, bad, states, every, 4, "loads is not finite at step 3, component 0, observation 9")
    for m in ("accumulation", "flux", "flux_scale", "conductivity"):
        same_refusal(ctx, assemble, loads, None, (m, "source", KEY), 4, f"grad_{m} needs states")

    def with_sweep():
        assemble()
        ctx._select_precond("sweep")

    same_refusal(ctx, with_sweep, loads, states, every, 5, "PFV_PRECOND_SWEEP")
    ctx._select_precond("jacobi")
    bf = g.get_all_boundary_faces()
    interior = np.flatnonzero(~np.isin(np.arange(g.num_faces), bf))
    labels = list(np.array(["dir", "neu", "dir"])[np.arange(bf.size) % 3])
    inner = pa.BoundaryCondition(g, bf, labels)
    inner.is_internal[[interior[6], interior[3]]] = True
    robin = list(labels)
    robin[4] = robin[9] = "rob"
    partial = dict(AD.problem(g)["par"], specified_cells=np.array([0, 1]))
    for par, status, word in ((dict(AD.problem(g)["par"], bc=pa.BoundaryCondition(g, bf, robin)), 5, "Robin"),
                              (dict(AD.problem(g)["par"], bc=inner), 5, f"face {interior[3]} "), (partial, 5, "partial")):
        ad_r, data_r = AD.discretized(lib, g, dict(pr, par=par), "mpfa")
        with pytest.raises(pa.PorefvError, match=word) as e:
            ad_r.adjoint(g, data_r, N, pr["acc"], loads, states, want=(KEY,))
        assert e.value.status == status
        if word != "Robin":  # (a Robin face is refused by the assembly already: nothing to call on)
            same_refusal(ad_r.context(g), lambda: ad_r._assemble(g, data_r, pr["acc"], None, pr["src"]), loads, states,
                         every, status, word)
    gp = UP.geo(pa.CartGrid([3, 3], [1.0, 1.0]))
    gp.periodic_face_map = np.vstack([np.flatnonzero(np.isclose(gp.face_centers[0], 0.0)),
                                      np.flatnonzero(np.isclose(gp.face_centers[0], 1.0))])
    with pytest.raises(pa.PorefvError) as e:
        pa.AdvectionDiffusion(KW, library=lib).adjoint(gp, pa.initialize_data({}, KW, AD.problem(gp)["par"]), N,
                                                       np.ones(gp.num_cells), np.zeros((N, gp.num_cells)),
                                                       np.zeros((N + 1, gp.num_cells)), want=(KEY,))
    assert e.value.status == 5 and "periodic" in e.value.message
    # ---- a step that does not converge: an error status, the mark still in the exact output, nothing faulted
    assemble()
    ctx._select_precond("jacobi")
    st, msg, done, untouched = raw(ctx, loads, states, (KEY, "c0", "multipliers"), maxit=1)
    assert (st, done, untouched) == (6, 0, True)
    with pytest.raises(RuntimeError, match="no assembled system"):
        ctx.solve()
    with pytest.raises(pa.PorefvError) as e:
        AA.adjoint(P, want=(KEY,), maxit=1, precond="jacobi")
    assert e.value.status == 6
    # after the refusals: the call itself goes through, with the bits of a handle that was never refused
    again, info = AA.adjoint(P, want=(KEY,), rtol=1e-13, precond="jacobi")
    fresh = setup(lib, "tets2", "mpfa")
    ref, _ = AA.adjoint(fresh, want=(KEY,), rtol=1e-13, precond="jacobi")
    assert info["steps_done"] == N and again[KEY].tobytes() == ref[KEY].tobytes()
    assemble()
    st, msg, done, untouched = raw(ctx, loads, states, (KEY,))
    assert (st, done, untouched) == (0, N, False)


def region_too_large(lib, n=128):
    """fan_grid_3d(128) (_mpfa_adjoint_cases.region_too_large): the region of hub and pole fits the LDS for
    ``discretize`` but not with the exact gradient's own arrays beside it: status 5 naming the node, before anything
    runs, nothing written; "conductivity" of the same handle is still to be had."""
    from tests._node_class_cases import fan_grid_3d

    g = fan_grid_3d(n)
    P = AA.setup(lib, None, "mpfa", g=g, pr=AD.problem(g))
    pr, ad, data, ctx = P["pr"], P["ad"], P["data"], P["ctx"]
    assert ctx.stats()["advdiff_adjoint_steps"] == 0
    with pytest.raises(pa.PorefvError, match=r"node [01] \(up to 128 sub-faces\)") as e:
        AA.adjoint(P, want=(KEY,))
    assert e.value.status == 5 and "LDS" in e.value.message
    ad._assemble(g, data, pr["acc"], None, pr["src"])
    st, msg, done, untouched = raw(ctx, np.ascontiguousarray(P["loads"]), np.ascontiguousarray(P["states"]), ALL + (KEY,))
    assert (st, done, untouched) == (5, 0, True) and "does not fit the LDS" in msg
    assert ctx.stats()["advdiff_adjoint_steps"] == 0  # (refused before its first solve)
    got, info = AA.adjoint(P, want=("conductivity", "source"))
    assert info["steps_done"] == N and np.abs(got["conductivity"]).max() > 0.0
