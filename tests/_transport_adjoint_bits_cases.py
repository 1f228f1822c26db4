"""The bits of the four transport adjoints (pfv_transport_adjoint_multi, _react, _nl, _nl_multi), pinned to a recording:
``record(lib)`` runs a few small calls of each through the public Python API and returns everything they give back
that is not a time, ``check(lib, fixture)`` records again and compares with the file to the byte.  The library uses no
floating-point atomics and fixes every summation order, so one build gives one answer; the fixtures under
tests/golden/transport_adjoint_bits hold it per build, ``emulation.npz`` for the host-emulated kernels (g++ -O2, no
contraction of multiply-adds) and ``gfx950.npz`` for the HIP library, both recorded before the four calls were moved
into one frame.  A change of the host code between the arguments and the gradients -- the order of the launches, a
buffer that is not zeroed, a slab staged into the wrong array, another acceptance -- shows here where the tolerances of
the case modules would let it pass.

Per call: tets(3) with three steps, every gradient wanted and five cells observed; the same observed on every cell;
no step at all; the smallest cyclic core, solved and refused (maxit = 1); for the saturation with components also
either kind of loads alone and the dry row.  The problems are those of the case modules; the states they compute go
through float32 on the way in, so that the last bits of numpy's and scipy's own arithmetic, which may differ from one
processor to the next, do not reach the library."""
import os

import numpy as np

import porepy_amd as pa
from tests import _adjoint_cases as A
from tests import _react_adjoint_cases as R
from tests import _satcomp_adjoint_cases as SC
from tests import _saturation_adjoint_cases as S
from tests._multi_cases import discretized
from tests._react_cases import chain_with_partner
from tests._saturation_cases import cfl_accumulation, core_problem, inflow_values
from tests._sweep_cases import cyclic_field
from tests._upwind_cases import tets

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "transport_adjoint_bits")
SWEEP_STATS = ("sweep_levels", "sweep_core_cells", "sweep_launches")


def coarse(x):
    """x through float32: inputs whose last bits the host's libraries decide"""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def _dense(p, loads, obs):
    """the loads on every cell: zeros off the observed ones"""
    out = np.zeros(loads.shape[:-1] + (p["g"].num_cells,))
    out[..., obs] = loads
    return out


def _note(rec, case, prefix, ctx, call):
    """One call into rec under ``case/``: the gradients, the info without its times, the sweep's and the call's
    counters; of a refusal the exception's kind, status and message, and what it carries of the info."""
    def info_in(info):
        for m, v in info.items():
            if m != "solve_ms":
                rec[f"{case}/info/{m}"] = np.asarray(v)

    try:
        grads, info = call()
    except (ValueError, pa.PorefvError) as e:
        rec[f"{case}/refused/kind"] = np.asarray(type(e).__name__)
        rec[f"{case}/refused/status"] = np.asarray(getattr(e, "status", -1))
        rec[f"{case}/refused/message"] = np.asarray(getattr(e, "message", str(e)))
        info_in(getattr(e, "info", {}))
    else:
        for m, v in grads.items():
            rec[f"{case}/grad/{m}"] = np.ascontiguousarray(v)
        info_in(info)
    st = ctx.stats()
    for m in SWEEP_STATS + (prefix + "_steps", prefix + "_core_iterations"):
        rec[f"{case}/stats/{m}"] = np.asarray(st[m])


def _five(rec, name, prefix, p, cyc, adjoint, loads=("loads",)):
    """the cases every call has: p on tets(3) with three steps, cyc on the cyclic core with two"""
    dense = dict(p, **{m: _dense(p, p[m], p["obs"]) for m in loads})
    ctx = p["up"].context(p["g"])
    _note(rec, f"{name}/observed", prefix, ctx, lambda: adjoint(p))
    _note(rec, f"{name}/every_cell", prefix, ctx, lambda: adjoint(dense, obs_cells=None))
    cctx = cyc["up"].context(cyc["g"])
    _note(rec, f"{name}/cyclic", prefix, cctx, lambda: adjoint(cyc))
    _note(rec, f"{name}/cyclic_refused", prefix, cctx, lambda: adjoint(cyc, maxit=1, raise_on_fail=False))
    _note(rec, f"{name}/cyclic_refused_raised", prefix, cctx, lambda: adjoint(cyc, maxit=1))


def _multi(lib, rec, k=3):
    g = tets(3)
    p = A.problem(lib, g, k, 3)
    p["states"] = coarse(p["states"])
    # the cyclic field of A.cyclic_core
    cg, q = cyclic_field()
    rng = np.random.default_rng(1)
    bf = cg.get_all_boundary_faces()
    bv = np.zeros((2, cg.num_faces))
    bv[:, bf] = rng.random((2, bf.size))
    vol = np.asarray(cg.cell_volumes, dtype=float)
    acc = np.array([vol * (0.5 + rng.random(cg.num_cells)) / 0.05 * (1.0 + 0.5 * a) for a in range(2)])
    c0 = rng.random((2, cg.num_cells))
    source = rng.random((2, cg.num_cells)) * vol
    obs = np.sort(rng.permutation(cg.num_cells)[:5])
    loads = rng.standard_normal((2, 2, 5))
    up, data = discretized(lib, cg, q, None, bv[0])
    states, _ = A.forward(up, cg, q, None, acc, bv, c0, source, 2)
    cyc = dict(g=cg, up=up, data=data, n_steps=2, acc=acc, loads=loads, obs=obs, states=coarse(states), bv=bv)
    _five(rec, "multi", "transport_adjoint", p, cyc, A.adjoint)
    p0 = A.problem(lib, g, k, 0)
    _note(rec, "multi/no_step", "transport_adjoint", p0["up"].context(g), lambda: A.adjoint(p0))


def _react(lib, rec, k=3):
    g = tets(3)
    p = R.problem(lib, g, k, 3)
    p["states"] = coarse(p["states"])
    # the cyclic field of R.cyclic_core
    cg, q = cyclic_field(12)
    nc = cg.num_cells
    K, w = chain_with_partner()
    kc = K.shape[0]
    rng = np.random.default_rng(5)
    acc0 = cfl_accumulation(cg, q, 2.0)
    acc = np.array([(1.0 + 0.5 * a) * acc0 for a in range(kc)])
    rho = acc0 * (0.5 + rng.random(nc))
    bv = np.array([(0.5 + 0.25 * a) * inflow_values(cg, 1.0) for a in range(kc)])
    c0 = 0.2 + rng.random((kc, nc))
    obs = np.sort(rng.permutation(nc)[:5])
    loads = rng.standard_normal((2, kc, 5))
    up, data = discretized(lib, cg, q, None, bv[0])
    M, bref = R.block_system(up, cg, q, None, acc, bv, K, w, rho)
    states = R.forward(M, bref, acc, c0, np.zeros((kc, nc)), w, 2)
    cyc = dict(g=cg, up=up, data=data, n_steps=2, acc=acc, K=K, w=w, rho=rho, loads=loads, obs=obs,
               states=coarse(states), bv=bv)
    _five(rec, "react", "transport_react_adjoint", p, cyc, R.adjoint)
    p0 = R.problem(lib, g, k, 0)
    _note(rec, "react/no_step", "transport_react_adjoint", p0["up"].context(g), lambda: R.adjoint(p0))


def _nl(lib, rec):
    p = S.tets_problem(lib, 3, 3)
    p["states"] = coarse(p["states"])
    cg, q, cfl, _, _ = core_problem("cyclic12")
    cyc = S.problem(lib, cg, q, 2, cfl=cfl)
    cyc["states"] = coarse(cyc["states"])
    _five(rec, "nl", "transport_nl_adjoint", p, cyc, S.adjoint)
    p0 = S.tets_problem(lib, 3, 0)
    _note(rec, "nl/no_step", "transport_nl_adjoint", p0["up"].context(p0["g"]), lambda: S.adjoint(p0))


def _nl_multi(lib, rec, k=3):
    name, prefix = "nl_multi", "transport_nlc_adjoint"
    p = SC.tets_problem(lib, 3, 3, k)
    p["s_states"], p["c_states"] = coarse(p["s_states"]), coarse(p["c_states"])
    cg, q, cfl, _, _ = core_problem("cyclic12")
    cyc = SC.problem(lib, cg, q, 2, 2, cfl=cfl)
    cyc["s_states"], cyc["c_states"] = coarse(cyc["s_states"]), coarse(cyc["c_states"])
    _five(rec, name, prefix, p, cyc, SC.adjoint, loads=("s_loads", "c_loads"))
    ctx = p["up"].context(p["g"])
    p0 = SC.tets_problem(lib, 3, 0, k)
    _note(rec, f"{name}/no_step", prefix, p0["up"].context(p0["g"]), lambda: SC.adjoint(p0))
    _note(rec, f"{name}/s_loads_only", prefix, ctx, lambda: SC.adjoint(p, c_loads=None))
    _note(rec, f"{name}/c_loads_only", prefix, ctx, lambda: SC.adjoint(p, s_loads=None))
    # the dry row of SC.refusals: a state that is exactly 0 and no sorption
    dry = p["s_states"].copy()
    dry[1, 7] = 0.0
    _note(rec, f"{name}/dry_row", prefix, ctx, lambda: SC.adjoint(p, s_states=dry, sorption=None))


def record(lib) -> dict:
    rec = {}
    for part in (_multi, _react, _nl, _nl_multi):
        part(lib, rec)
    return rec


def check(lib, fixture):
    """record(lib) against tests/golden/transport_adjoint_bits/<fixture>: the same entries, each of the same type, shape
    and bytes"""
    rec = record(lib)
    with np.load(os.path.join(GOLDEN, fixture)) as f:
        want = {m: f[m] for m in f.files}
    assert sorted(rec) == sorted(want)
    differ = [m for m in sorted(want) if rec[m].dtype != want[m].dtype or rec[m].shape != want[m].shape
              or rec[m].tobytes() != want[m].tobytes()]
    assert not differ, differ
    # what the recording must contain to pin anything: gradients that are not zero, the refusals as refusals
    for call in ("multi", "react", "nl", "nl_multi"):
        assert any(want[m].any() for m in want if m.startswith(f"{call}/observed/grad/"))
        assert want[f"{call}/cyclic/info/steps_done"] == 2 and want[f"{call}/cyclic_refused/info/steps_done"] == 0
        assert not any(want[m].any() for m in want if m.startswith(f"{call}/cyclic_refused/grad/"))
        assert want[f"{call}/cyclic_refused_raised/refused/status"] == 6
    assert "is dry" in str(want["nl_multi/dry_row/refused/message"])
