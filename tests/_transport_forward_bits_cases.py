"""The bits of the flow-ordered forward transport steps (pfv_transport_advance_multi, _nl, _nl_multi, _react), pinned to
a recording as tests/_transport_adjoint_bits_cases.py pins the four adjoints: ``record(lib)`` runs a few small calls of
each through the public Python API and returns everything they give back that is not a time, ``check(lib, fixture)``
records again and compares with the file to the byte.  The fixtures under tests/golden/transport_forward_bits hold one
answer per build, ``emulation.npz`` for the host-emulated kernels and ``gfx950.npz`` for the HIP library, both recorded
at 448225e, before the three calls were moved into the set-up, the step frame and the sweep solve of the adjoints.  A
change of the host code between the arguments and the states -- the order of the launches, a buffer that is not
zeroed, another acceptance, a counter that moves -- shows here where the tolerances of the case modules let it pass.

Per call: tets(3) with three steps; no step at all; the smallest cyclic core with two steps, solved, refused
(maxit = 1) and the refusal raised; one refusal of the inputs with two offenders.  Beside these the branches only one
call has (``_multi``, ``_nl_multi``, ``_react``).  The problems are those of the case modules; whatever numpy or scipy
computed of them goes through float32 on the way in, so that the last bits of their arithmetic, which may differ from
one processor to the next, do not reach the library."""
import os

import numpy as np

import porepy_amd as pa
from tests import _multi_cases as M
from tests import _react_cases as R
from tests import _satcomp_cases as SC
from tests import _saturation_cases as S
from tests._sweep_cases import VEL, cyclic_field, edges, flow_order
from tests._upwind_cases import KW, data_for, line_grid, tets

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transport_forward_bits")
STATS = ("sweep_levels", "sweep_core_cells", "sweep_launches", "sweep_direct_steps",
         "transport_iterations", "transport_gmres_retries",
         "transport_multi_components", "transport_multi_direct_steps", "transport_multi_fallback_components",
         "transport_nl_steps", "transport_nl_core_iterations", "transport_nl_components",
         "transport_react_steps", "transport_react_core_iterations", "transport_react_components")
CALLS = ("multi", "nl", "nl_multi", "react")


def coarse(x):
    """x through float32: inputs whose last bits the host's libraries decide"""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _note(rec, case, ctx, names, call, start=None):
    """One call into rec under ``case/``: the states it returns under ``names``, the info without its times, the
    counters in the order of STATS (one array: the fixture's size is that of its entries); of a refusal the exception's
    kind, status and message, and what it carries of the state and the info.  ``start``: the state the call starts
    from, kept where check() compares with it."""
    def info_in(info):
        for m, v in (info or {}).items():
            if m != "solve_ms":
                rec[f"{case}/info/{m}"] = np.asarray(v)

    def states_in(states):
        for m, v in zip(names, states):
            rec[f"{case}/out/{m}"] = np.ascontiguousarray(v)

    for m, v in zip(names, start or ()):
        rec[f"{case}/start/{m}"] = np.ascontiguousarray(v, dtype=np.float64)
    try:
        *states, info = call()
    except (ValueError, pa.PorefvError) as e:
        rec[f"{case}/refused/kind"] = np.asarray(type(e).__name__)
        rec[f"{case}/refused/status"] = np.asarray(getattr(e, "status", -1))
        rec[f"{case}/refused/message"] = np.asarray(getattr(e, "message", str(e)))
        state = getattr(e, "state", None)
        if state is not None:
            states_in(state if isinstance(state, tuple) else (state,))
        info_in(getattr(e, "info", None))
    else:
        states_in(states)
        info_in(info)
    st = ctx.stats()
    rec[f"{case}/stats"] = np.array([st[m] for m in STATS], dtype=np.int64)


def _common(rec, name, names, acyclic, cyclic):
    """the cases every call has.  acyclic = (up, g, start, run) on tets(3), cyclic the same on the smallest core;
    run(n_steps, **kw) is the call"""
    up, g, start, run = acyclic
    ctx = up.context(g)
    _note(rec, f"{name}/tets", ctx, names, lambda: run(3), start)
    _note(rec, f"{name}/no_step", ctx, names, lambda: run(0), start)
    up, g, start, run = cyclic
    ctx = up.context(g)
    _note(rec, f"{name}/cyclic", ctx, names, lambda: run(2), start)
    _note(rec, f"{name}/cyclic_refused", ctx, names, lambda: run(2, maxit=1, raise_on_fail=False), start)
    _note(rec, f"{name}/cyclic_refused_raised", ctx, names, lambda: run(2, maxit=1))


def _changed(x, where):
    y = np.array(x, dtype=np.float64, copy=True)
    for idx, v in where.items():
        y[idx] = v
    return y


# ---- pfv_transport_advance_multi -------------------------------------------------------------------------------------------
def _multi_problem(g, k):
    q, bc, acc, bv, c0, source = M.components(g, k)
    return coarse(q), bc, coarse(acc), bv, c0, source


def _multi(lib, rec, k=3):
    g = tets(3)
    q, bc, acc, bv, c0, source = _multi_problem(g, k)
    up, data = M.discretized(lib, g, q, bc, bv[0])
    ctx = up.context(g)

    def run(n_steps, c=c0, a=acc, b=bv, src=source, d=data, **kw):
        kw.setdefault("precond", "sweep")
        return up.advance_components(g, d, c, n_steps, a, bc_values=b, source=src, **kw)

    # the cyclic field of M.core_takes_the_component_path: a core sends every component through its own Krylov solves
    cg, cq = cyclic_field()
    cq = coarse(cq)
    rng = np.random.default_rng(1)
    bf = cg.get_all_boundary_faces()
    cbv = np.zeros((2, cg.num_faces))
    cbv[:, bf] = rng.random((2, bf.size))
    vol = np.asarray(cg.cell_volumes, dtype=float)
    cacc = coarse(np.array([vol * (0.5 + rng.random(cg.num_cells)) / 0.05 * (1.0 + 0.5 * a) for a in range(2)]))
    cc0 = rng.random((2, cg.num_cells))
    cup, cdata = M.discretized(lib, cg, cq, None, cbv[0])

    def crun(n_steps, **kw):
        return cup.advance_components(cg, cdata, cc0, n_steps, cacc, bc_values=cbv, precond="sweep", method="gmres", **kw)

    _common(rec, "multi", ("c",), (up, g, (c0,), run), (cup, cg, (cc0,), crun))
    # the slow path: Jacobi and BiCGStab (the component from rest breaks BiCGStab down); then one component that stops
    # early, so that all are taken again up to the step it reached
    _note(rec, "multi/jacobi", ctx, ("c",), lambda: run(2, precond="jacobi"), (c0,))
    # (Component 0 starts with a blob in a cell of the last level that leaves within a step: its right-hand side shrinks by
    # three decades per step, and with it what rtol allows the rest -- 2, 7 and 11 GMRES iterations for the three steps,
    # 3 and 4 at every step for the others, whose accumulation is 16-fold.  maxit = 9 stops component 0 in the third.)
    level = flow_order(g.num_cells, *edges(g, q))["level"]
    last = int(np.flatnonzero(level == level.max())[0])
    blob, thin = _changed(c0, {(0, last): 1e9}), _changed(acc, {1: 16.0 * acc[1], 2: 16.0 * acc[2], (0, last): 1e-3 * acc[0, last]})
    _note(rec, "multi/target_shrinks", ctx, ("c",),
          lambda: run(3, c=blob, a=thin, precond="jacobi", method="gmres", rtol=1e-6, maxit=9, raise_on_fail=False), (blob,))
    # the fast path with a flux that contradicts the discretization's on four faces (M.failed_check_falls_back): the
    # components that carry something across them fail the check and are solved alone; the last one is zero throughout
    z0, zsrc = _changed(c0, {k - 1: 0.0}), _changed(source, {k - 1: 0.0})
    interior = np.setdiff1d(np.arange(g.num_faces), g.get_all_boundary_faces())
    flip = interior[np.random.default_rng(9).permutation(interior.size)[:4]]
    q2 = q.copy()
    q2[flip] = -q2[flip]
    _note(rec, "multi/check_falls_back", ctx, ("c",),
          lambda: run(1, c=z0, a=4.0 * acc, src=zsrc, d=data_for(q2, bc, bv[0]), method="gmres", rtol=1e-11), (z0,))
    # a right-hand side that is exactly zero (no state, no inflow value, no source): converged whatever the sweep left
    _note(rec, "multi/zero_rhs", ctx, ("c",),
          lambda: run(2, c=_changed(c0, {1: 0.0}), b=_changed(bv, {1: 0.0}), src=_changed(source, {1: 0.0})))
    # a zero diagonal (M.errors: cell 2 of the line has no outflow) in two components: the lower one is named
    g1 = line_grid(6, 1.0)
    q1 = np.where(g1.face_centers[0] < 0.5, 1.0, -1.0)
    d1 = data_for(q1, None, np.zeros(g1.num_faces))
    up1 = pa.Upwind(KW, library=lib)
    up1.discretize(g1, d1)
    acc1 = _changed(np.ones((3, 6)), {(1, 2): 0.0, (2, 2): 0.0})
    _note(rec, "multi/inputs_refused", up1.context(g1), ("c",),
          lambda: up1.advance_components(g1, d1, np.zeros((3, 6)), 2, acc1, precond="sweep"))


# ---- pfv_transport_advance_nl, pfv_transport_advance_nl_multi -----------------------------------------------------------------
def _saturation_problem(lib, g, q, cfl):
    q = coarse(q)
    bv, acc = S.inflow_values(g), coarse(S.cfl_accumulation(g, q, cfl))
    up, data = S.discretized(lib, g, q, bv)
    return up, data, acc


def _nl(lib, rec):
    ff = S.corey()
    g = tets(3)
    up, data, acc = _saturation_problem(lib, g, pa.Upwind(KW).darcy_flux(g, VEL), 5.0)
    s0 = np.full(g.num_cells, 0.1)

    def run(n_steps, s=s0, a=acc, **kw):
        return up.advance_saturation(g, data, s, n_steps, a, ff, **kw)

    cg, cq, cfl, cs0, _ = S.core_problem("cyclic12")
    cup, cdata, cacc = _saturation_problem(lib, cg, cq, cfl)

    def crun(n_steps, **kw):
        return cup.advance_saturation(cg, cdata, cs0, n_steps, cacc, ff, **kw)

    _common(rec, "nl", ("s",), (up, g, (s0,), run), (cup, cg, (cs0,), crun))
    # the rotation, whose core is the whole grid: what nl_multi/frozen is compared with
    rg, rq, rcfl, rs0, _ = S.core_problem("rotation8")
    rup, rdata, racc = _saturation_problem(lib, rg, rq, rcfl)
    _note(rec, "nl/rotation", rup.context(rg), ("s",), lambda: rup.advance_saturation(rg, rdata, rs0, 2, racc, ff))
    _note(rec, "nl/inputs_refused", up.context(g), ("s",), lambda: run(1, a=_changed(acc, {5: 0.0, 9: -1.0})))


def _nl_multi(lib, rec, k=3):
    ff = S.corey()
    g = tets(3)
    up, data, acc = _saturation_problem(lib, g, pa.Upwind(KW).darcy_flux(g, VEL), 5.0)
    s0 = np.full(g.num_cells, 0.1)
    cbv, c0, ads, csrc = SC.tets_components(g, acc, k)

    def run(n_steps, **kw):
        for m, v in (("c_bc_values", cbv), ("sorption", ads), ("c_source", csrc)):
            kw.setdefault(m, v)
        return up.advance_saturation_components(g, data, s0, c0, n_steps, acc, ff, **kw)

    def core(which):  # SC._core_setup(which, k)
        cg, cq, cfl, cs0, _ = S.core_problem(which)
        cup, cdata, cacc = _saturation_problem(lib, cg, cq, cfl)
        rng = np.random.default_rng(5)
        ccbv = np.zeros((k, cg.num_faces))
        ccbv[:, cg.get_all_boundary_faces()] = (0.5 + np.arange(k))[:, None]
        cc0 = 0.2 + rng.random((k, cg.num_cells))
        cads = _changed(np.zeros((k, cg.num_cells)), {0: 0.3 * cacc})

        def crun(n_steps, **kw):
            return cup.advance_saturation_components(cg, cdata, cs0, cc0, n_steps, cacc, ff, c_bc_values=ccbv,
                                                     sorption=cads, **kw)

        return cup, cg, (cs0, cc0), crun

    names = ("s", "c")
    _common(rec, "nl_multi", names, (up, g, (s0, c0), run), core("cyclic12"))
    # on the rotation the components go on iterating after the saturation has passed its own test (SC.saturation_unchanged;
    # check() compares the core iterations with those of nl/rotation, the same saturation alone)
    rup, rg, _, rrun = core("rotation8")
    _note(rec, "nl_multi/frozen", rup.context(rg), names, lambda: rrun(2))
    ctx = up.context(g)
    _note(rec, "nl_multi/no_sorption", ctx, names, lambda: run(3, sorption=None))
    _note(rec, "nl_multi/no_c_source", ctx, names, lambda: run(3, c_source=None))
    _note(rec, "nl_multi/inputs_refused", ctx, names,
          lambda: run(1, sorption=_changed(ads, {(1, 5): -1e-3, (0, 9): -1.0})))


# ---- pfv_transport_advance_react ---------------------------------------------------------------------------------------------
def _react_problem(lib, k):
    g, q, bc, acc, bv, c0, source, K, w, rho = R.tets_problem(3, k)
    q, acc, rho = coarse(q), coarse(acc), coarse(rho)
    up, data = M.discretized(lib, g, q, bc, bv[0])

    def run(n_steps, c=c0, a=acc, **kw):
        for m, v in (("rate_weight", rho), ("mobility", w), ("bc_values", bv), ("source", source)):
            kw.setdefault(m, v)
        return up.advance_reactive_components(g, data, c, n_steps, a, K, **kw)

    return up, g, c0, acc, run


def _react(lib, rec, k=3):
    up, g, c0, acc, run = _react_problem(lib, k)
    # the core of R.core_case("cyclic12-k3")
    cg, cq = cyclic_field(12)
    cq = coarse(cq)
    nc = cg.num_cells
    K, w = R.network(k)
    rng = np.random.default_rng(5)
    acc0 = coarse(S.cfl_accumulation(cg, cq, 2.0))
    cacc = np.array([(1.0 + 0.5 * a) * acc0 for a in range(k)])
    rho = coarse(acc0 * (0.5 + rng.random(nc)))
    cbv = np.array([(0.5 + 0.25 * a) * S.inflow_values(cg, 1.0) for a in range(k)])
    cc0 = 0.2 + rng.random((k, nc))
    cup, cdata = M.discretized(lib, cg, cq, None, cbv[0])

    def crun(n_steps, **kw):
        return cup.advance_reactive_components(cg, cdata, cc0, n_steps, cacc, K, rate_weight=rho, mobility=w,
                                               bc_values=cbv, **kw)

    _common(rec, "react", ("c",), (up, g, (c0,), run), (cup, cg, (cc0,), crun))
    ctx = up.context(g)
    _note(rec, "react/no_rate_weight", ctx, ("c",), lambda: run(3, rate_weight=None))
    _note(rec, "react/inputs_refused", ctx, ("c",), lambda: run(1, a=_changed(acc, {(2, 11): 0.0, (0, 40): 0.0})))
    # an accumulation that is not finite passes the check of the inputs (it is positive): the block of its cell has a
    # pivot that is not finite, which the finished sweep reports
    inf_acc = _changed(acc, {(1, 5): np.inf})
    _note(rec, "react/pivot", ctx, ("c",), lambda: run(2, a=inf_acc, raise_on_fail=False), (c0,))
    _note(rec, "react/pivot_raised", ctx, ("c",), lambda: run(2, a=inf_acc))
    # the chain with its immobile partner (k = 4, mobility 1, 1, 1, 0)
    up4, g4, c4, _, run4 = _react_problem(lib, 4)
    _note(rec, "react/immobile", up4.context(g4), ("c",), lambda: run4(3), (c4,))


def record(lib) -> dict:
    rec = {}
    for part in (_multi, _nl, _nl_multi, _react):
        part(lib, rec)
    return rec


def check(lib, fixture):
    """record(lib) against tests/golden/transport_forward_bits/<fixture>: the same entries, each of the same type, shape
    and bytes"""
    rec = record(lib)
    with np.load(os.path.join(GOLDEN, fixture)) as f:
        want = {m: f[m] for m in f.files}
    assert sorted(rec) == sorted(want)
    differ = [m for m in sorted(want) if rec[m].dtype != want[m].dtype or rec[m].shape != want[m].shape
              or rec[m].tobytes() != want[m].tobytes()]
    assert not differ, differ

    # what the recording must contain to pin anything: states that moved, the refusals as refusals
    def stat(case, m):
        return want[f"{case}/stats"][STATS.index(m)]

    def unchanged(case):
        return all(want[m].tobytes() == want[m.replace("/out/", "/start/")].tobytes()
                   for m in want if m.startswith(f"{case}/out/"))

    for call in CALLS:
        assert want[f"{call}/tets/info/steps_done"] == 3 and not unchanged(f"{call}/tets")
        assert want[f"{call}/no_step/info/steps_done"] == 0 and unchanged(f"{call}/no_step")
        assert want[f"{call}/cyclic/info/steps_done"] == 2 and not unchanged(f"{call}/cyclic")
        assert stat(f"{call}/cyclic", "sweep_core_cells") == 45
        assert want[f"{call}/cyclic_refused/info/steps_done"] == 0 and unchanged(f"{call}/cyclic_refused")
        assert want[f"{call}/cyclic_refused_raised/refused/status"] == 6
    # the lower of the two offenders.  What the checks of the inputs refuse has status 4, which Upwind turns into a
    # ValueError with the library's words; the zero diagonal of multi is "unsupported" (5) and stays a PorefvError
    for call, kind, status, text in (("multi", "PorefvError", 5, "zero diagonal entry in row 2, component 1 "),
                                     ("nl", "ValueError", -1, "accumulation must be positive: cell 5"),
                                     ("nl_multi", "ValueError", -1, "sorption must not be negative: cell 5, component 1"),
                                     ("react", "ValueError", -1, "accumulation must be positive: cell 11, component 2")):
        assert want[f"{call}/inputs_refused/refused/kind"] == kind
        assert want[f"{call}/inputs_refused/refused/status"] == status
        assert str(want[f"{call}/inputs_refused/refused/message"]).startswith(text)
    # multi: the component path of the core and of Jacobi, the fallback of single components, the shrinking target
    assert stat("multi/tets", "transport_multi_direct_steps") == 3
    assert stat("multi/cyclic", "transport_multi_fallback_components") == 2 * 2
    assert stat("multi/jacobi", "transport_multi_fallback_components") == 3 * 2
    assert stat("multi/jacobi", "transport_gmres_retries") >= 1
    assert want["multi/target_shrinks/info/steps_done"] == 2 and not unchanged("multi/target_shrinks")
    assert 1 <= stat("multi/check_falls_back", "transport_multi_fallback_components") <= 2
    assert want["multi/check_falls_back/info/steps_done"] == 1 and not unchanged("multi/check_falls_back")
    assert want["multi/zero_rhs/info/steps_done"] == 2 and not want["multi/zero_rhs/out/c"][1].any()
    assert want["multi/zero_rhs/info/converged"].all() and want["multi/zero_rhs/info/rel_residual"][1] == 0.0
    # nl_multi: the components iterate on after the saturation has frozen
    assert want["nl_multi/frozen/info/steps_done"] == 2 and stat("nl_multi/frozen", "sweep_core_cells") == 64
    assert stat("nl_multi/frozen", "transport_nl_core_iterations") > stat("nl/rotation", "transport_nl_core_iterations")
    for case, alone in (("cyclic", "cyclic"), ("frozen", "rotation")):
        assert want[f"nl_multi/{case}/out/s"].tobytes() == want[f"nl/{alone}/out/s"].tobytes()
    for case in ("no_sorption", "no_c_source"):
        assert want[f"nl_multi/{case}/info/steps_done"] == 3
        assert want[f"nl_multi/{case}/out/c"].tobytes() != want["nl_multi/tets/out/c"].tobytes()
    # react
    assert want["react/pivot_raised/refused/status"] == 6
    assert "the block of cell 5 has a pivot that is not positive and finite" in str(want["react/pivot_raised/refused/message"])
    assert want["react/pivot/info/steps_done"] == 0 and unchanged("react/pivot")
    assert want["react/no_rate_weight/out/c"].tobytes() != want["react/tets/out/c"].tobytes()
    assert want["react/immobile/info/steps_done"] == 3 and not unchanged("react/immobile")

