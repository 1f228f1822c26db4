"""Times of the resident transport chain on the headline grid (6 * n^3 tetrahedra, n = 69: 1 971 054 cells), next to
the same chain on the host with scipy, measured in the same run:

    face flux -> upwind discretize -> assemble -> 20 implicit Euler steps

Device times are HIP-event times from pfv_stats; the host times are wall clock.  Prints one JSON line.  A measurement,
not a test: no thresholds.

    python tools/bench_transport.py [--n-side 69] [--steps 20] [--no-host] [--precond sweep] [--components 8]
                                    [--saturation [--components 4]] [--reactive] [--adjoint]
                                    [--reactive --adjoint] [--saturation --adjoint] [--sorbing [--components 1,4,16]]

--precond sweep: after the Jacobi-BiCGStab steps, the same steps from the same state with the flow-ordered sweep
(PFV_PRECOND_SWEEP) -- order-build ms, levels, core cells, launches per sweep, ms per step -- and again with one launch
per level (PFV_SWEEP_MERGE=0); both figures of the comparison come from this one run on the same inputs.

--components K (with --precond sweep; a comma-separated list runs several K): K quantities with retardation 1 + a / 2
and their own inflow values, first as K single assemble + advance(precond="sweep") runs, then as ONE
transport_advance_multi from the same state on the same handle: ms per step of both (HIP events, best and median of
--reps), levels and launches per sweep, and the largest difference between the two results.

--saturation: on the same flux and from the same state, the linear sweep steps (advance with precond="sweep") and then
the same number of saturation steps with a Corey curve (transport_advance_nl: exponents 2 / 2, viscosities 1 / 5,
residual saturations 0.1 / 0.15): ms per step of both from pfv_stats (best and median of --reps, the first repeat
dropped), levels, launches, core cells and core iterations.

--saturation --components K (a list runs several K): in addition, alternating in one loop from the same state, the
Corey step alone, the Corey step with K phase-carried components (transport_advance_nl_multi: own inflow concentrations,
sorption on component 0) and, for orientation, the K-component linear step (transport_advance_multi with
precond="sweep"): ms per step of the three (best and median of --reps, the first repeat dropped), levels, launches.

--reactive: alternating in one loop from the same state, the k = 4 steps of the linear multi-component sweep
(transport_advance_multi with precond="sweep") and the same number of reactive k = 4 steps (transport_advance_react):
the chain 0 -> 1 -> 2 plus the exchange 0 <-> 3 with component 3 immobile, the reaction term weighted by the pore
volume.  ms per step of both from pfv_stats (best and median of --reps, the first repeat dropped), levels, launches.

--sorbing (JSON key "sorbing"): alternating in one loop from the same non-negative state, the k = 4 steps of the linear
multi-component sweep (transport_advance_multi with precond="sweep"), the same number of sorbing k = 4 steps
(transport_advance_sorb) with the components Freundlich n = 0.5, Freundlich n = 0.7, Langmuir and linear and a capacity
of half the accumulation, and the sorbing call with four LINEAR components (Kd = 1: the linear step with the folded
accumulation).  ms per step of the three from pfv_stats (best and median of --reps, the first repeat dropped), levels,
launches.  --sorbing --components K (a list runs several K): in addition the sorbing step with K components that cycle
those four isotherms, ms per step.

--adjoint: in the same process and on the same flux, alternating in one loop, the forward k = 4 sweep step
(transport_advance_multi with precond="sweep") and the adjoint k = 4 step (transport_adjoint_multi) on 16 observation
cells -- once with the three gradients that need no states (c0, source, bc_values) and once with all five, which stages
one slab of states per step: ms per step of the three from pfv_stats (best and median of --reps, the first repeat
dropped), the launches of the sweep and the other kernels per step for both directions.

--reactive --adjoint (together; the two blocks above are then NOT run, and the JSON has the key "reactive_adjoint" in
place of "reactive" and "adjoint"): alternating in one loop, the forward reactive
k = 4 step of --reactive's network (transport_advance_react), its adjoint (transport_adjoint_react) on 16 observation
cells without states (c0, source, bc_values) and the adjoint with all seven gradients: ms per step of the three from
pfv_stats (best and median of --reps, the first repeat dropped), levels and launches.

--saturation --adjoint (together; the blocks of --saturation and of --adjoint are then NOT run, and the JSON has the key
"saturation_adjoint" in their place): alternating in one loop, on the same flux, the forward Corey saturation step of
--saturation's curve with a sink (transport_advance_nl) from a random state in [0.15, 0.65], its adjoint
(transport_adjoint_nl) on 16 observation cells with the three gradients whose formulas need no states (s0, source,
bc_values) and the adjoint with all seven; the states are those of the forward run, taken one step at a time.  ms per
step of the three from pfv_stats (best and median of --reps, the first repeat dropped), levels and launches.

--saturation --adjoint --components K (a list runs several K; the JSON gains the key "satcomp_adjoint"): after the
block above and by its protocol, on the same flux, curve and sink, alternating in one loop: the forward Corey step with K
phase-carried components (transport_advance_nl_multi: own inflow concentrations, sorption on component 0), its adjoint
(transport_adjoint_nl_multi) on the same 16 observation cells with loads of both kinds and the four default gradients
(s0, c0, source, c_source), and the adjoint with all eleven.  ms per step of the three from pfv_stats (best, median and
worst of --reps, the first repeat dropped), levels and launches of both directions.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import porepy_amd as pa  # noqa: E402
from porepy_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-side", type=int, default=69)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--precond", choices=["jacobi", "sweep"], default="jacobi",
                    help="sweep: also time the steps with the flow-ordered sweep, next to the Jacobi-BiCGStab ones")
    ap.add_argument("--components", default="",
                    help="K or K1,K2,...: K single sweep runs against one multi-component run (with --precond sweep); "
                         "the Corey step alone against the Corey step with K components (with --saturation)")
    ap.add_argument("--saturation", action="store_true",
                    help="linear sweep steps against Corey saturation steps on the same flux and state")
    ap.add_argument("--reactive", action="store_true",
                    help="the linear k = 4 sweep steps against k = 4 coupled (reactive) steps on the same flux and state")
    ap.add_argument("--sorbing", action="store_true",
                    help="the linear k = 4 sweep steps against k = 4 sorbing steps (nonlinear isotherms) on the same flux "
                         "and state; with --components: also the sorbing step at those k")
    ap.add_argument("--adjoint", action="store_true",
                    help="the forward k = 4 sweep step against the adjoint k = 4 step on the same flux; with --saturation: "
                         "the forward Corey step against its adjoint")
    ap.add_argument("--emulation", action="store_true", help="run on the host-emulation build (plumbing check)")
    a = ap.parse_args()
    lib = None
    if a.emulation:
        from tests import _parity as P

        lib = P.emulation_library()
    n = a.n_side
    g = pa.StructuredTetrahedralGrid([n, n, n], [1.0, 1.0, 1.0])
    g.compute_geometry()
    g = pa.perturb_interior_nodes(g, 0.2 / n)
    nc, nf = g.num_cells, g.num_faces
    rng = np.random.default_rng(0)
    k = 1 + rng.random(nc)
    K = pa.SecondOrderTensor(kxx=k, kyy=1.5 * k, kzz=0.7 * k, kxy=0.1 * k)
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)
    fbv = np.zeros(nf)
    fbv[bf] = g.face_centers[:, bf].sum(axis=0)
    fdata = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": bc, "bc_values": fbv})
    ctx = pa.Context(0, lib)
    ctx.set_grid(pa.grid_to_raw(g))
    ctx.set_params(K.values, pa.bc_flags(bc), None, 1.0 / 3.0, None)
    ctx.discretize(rebuild_topology=True, skip_vector_source=True)
    ctx.assemble(fbv)
    p, info = ctx.solve("bicgstab", rtol=1e-10, maxit=20000, precond="amg", raise_on_fail=False)
    out = {"cells": nc, "faces": nf, "flow_iterations": info["iterations"], "flow_assemble_ms": ctx.stats()["assemble_ms"]}
    tbv = np.zeros(nf)
    tbv[bf] = rng.random(bf.size)
    dt = 0.5 / n  # about one cell per step at unit velocity
    acc = 0.2 * g.cell_volumes / dt
    c0 = np.zeros(nc)

    def best(fn, key):
        vals = []
        for _ in range(a.reps):
            fn()
            vals.append(ctx.stats()[key])
        return min(vals), float(np.median(vals))

    out["face_flux_ms"] = best(lambda: ctx.face_flux(p, fbv, out=False), "face_flux_ms")
    ctx.upwind_set_bc(None)
    out["upwind_discretize_ms"] = best(lambda: ctx.upwind_discretize(None, 1), "upwind_ms")
    out["transport_assemble_ms"] = best(lambda: ctx.upwind_assemble(tbv, None, accumulation=acc), "transport_assemble_ms")
    c, ainfo = ctx.transport_advance(c0, a.steps, rtol=1e-10, raise_on_fail=False)
    st = ctx.stats()
    out["advance"] = {"steps_done": ainfo["steps_done"], "ms_per_step": st["transport_advance_ms"] / max(a.steps, 1),
                      "iterations_per_step": st["transport_iterations"] / max(a.steps, 1)}
    if a.precond == "sweep":
        for key, merge in (("advance_sweep", "1"), ("advance_sweep_one_launch_per_level", "0")):
            os.environ["PFV_SWEEP_MERGE"] = merge
            cs, sinfo = ctx.transport_advance(c0, a.steps, rtol=1e-10, raise_on_fail=False, precond="sweep")
            first = ctx.stats()  # (the first call builds the order)
            cs, sinfo = ctx.transport_advance(c0, a.steps, rtol=1e-10, raise_on_fail=False, precond="sweep")
            ss = ctx.stats()
            out[key] = {"steps_done": sinfo["steps_done"], "ms_per_step": ss["transport_advance_ms"] / max(a.steps, 1),
                        "ms_per_step_first_call": first["transport_advance_ms"] / max(a.steps, 1),
                        "order_build_ms": first["sweep_order_ms"], "levels": ss["sweep_levels"],
                        "core_cells": ss["sweep_core_cells"], "launches_per_sweep": ss["sweep_launches"],
                        "direct_steps": ss["sweep_direct_steps"], "direct_fallbacks": ss["sweep_direct_fallbacks"],
                        "rel_residual_last_step": sinfo["rel_residual"],
                        "max_diff_to_jacobi_bicgstab": float(np.abs(cs - c).max())}
        del os.environ["PFV_SWEEP_MERGE"]
        out["components"] = []
        for kc in [int(v) for v in a.components.split(",") if v]:
            acc_k = np.array([(1.0 + 0.5 * j) * acc for j in range(kc)])
            bv_k = np.array([tbv * (j + 1) / kc for j in range(kc)])
            c0_k = rng.random((kc, nc))
            single_ms, multi_ms = [], []
            for _ in range(a.reps + 1):  # (the first repeat warms up and is dropped)
                ms, cs_k = 0.0, np.empty_like(c0_k)
                for j in range(kc):
                    ctx.upwind_assemble(bv_k[j], None, accumulation=acc_k[j])
                    ms += ctx.stats()["transport_assemble_ms"]
                    cs_k[j], sinfo = ctx.transport_advance(c0_k[j], a.steps, rtol=1e-10, raise_on_fail=False, precond="sweep")
                    ms += ctx.stats()["transport_advance_ms"]
                single_stats = ctx.stats()
                single_ms.append(ms / max(a.steps, 1))
                cm_k, minfo = ctx.transport_advance_multi(c0_k, a.steps, acc_k, bv_k, rtol=1e-10, raise_on_fail=False,
                                                          precond="sweep")
                ms_ = ctx.stats()
                multi_ms.append(ms_["transport_advance_ms"] / max(a.steps, 1))
            single_ms, multi_ms = single_ms[1:], multi_ms[1:]
            out["components"].append({
                "k": kc, "steps_done": minfo["steps_done"],
                "single_runs_ms_per_step": (min(single_ms), float(np.median(single_ms))),
                "multi_ms_per_step": (min(multi_ms), float(np.median(multi_ms))),
                "levels": ms_["sweep_levels"], "launches_per_sweep": ms_["sweep_launches"],
                "launches_per_sweep_single": single_stats["sweep_launches"],
                "direct_steps": ms_["transport_multi_direct_steps"],
                "fallback_components": ms_["transport_multi_fallback_components"],
                "max_rel_residual_last_step": max(minfo["rel_residual"]),
                "max_diff_multi_to_single": float(np.abs(cm_k - cs_k).max())})
        if a.components:
            ctx.upwind_assemble(tbv, None, accumulation=acc)  # (the multi-component call leaves no system behind)
    if a.saturation and not a.adjoint:
        s0 = np.full(nc, 0.1)
        corey = pa.CoreyFractionalFlow(s_wr=0.1, s_nr=0.15, n_w=2.0, n_n=2.0, mu_w=1.0, mu_n=5.0)
        lin_ms, nl_ms, sat = [], [], {}
        for _ in range(a.reps + 1):  # (the first repeat builds the order and warms up: dropped)
            cl, linfo = ctx.transport_advance(s0, a.steps, rtol=1e-10, raise_on_fail=False, precond="sweep")
            ls = ctx.stats()
            lin_ms.append(ls["transport_advance_ms"] / max(a.steps, 1))
        try:
            for _ in range(a.reps + 1):
                sn, ninfo = ctx.transport_advance_nl(s0, a.steps, acc, tbv, corey.kind, corey.params, rtol=1e-10,
                                                     raise_on_fail=False)
                ns = ctx.stats()
                nl_ms.append(ns["transport_nl_ms"] / max(a.steps, 1))
            sat = {"steps_done": ninfo["steps_done"], "corey_ms_per_step": (min(nl_ms[1:]), float(np.median(nl_ms[1:]))),
                   "levels": ns["sweep_levels"], "core_cells": ns["sweep_core_cells"],
                   "launches_per_step": ns["sweep_launches"], "core_iterations": ns["transport_nl_core_iterations"],
                   "rel_residual_last_step": ninfo["rel_residual"], "s_min": float(sn.min()), "s_max": float(sn.max())}
        except pa.PorefvError as e:
            sat = {"error": e.message, "core_cells": ctx.stats()["sweep_core_cells"], "levels": ctx.stats()["sweep_levels"]}
        sat.update({"linear_sweep_ms_per_step": (min(lin_ms[1:]), float(np.median(lin_ms[1:]))),
                    "linear_steps_done": linfo["steps_done"], "linear_direct_steps": ls["sweep_direct_steps"],
                    "linear_launches_per_sweep": ls["sweep_launches"], "linear_core_cells": ls["sweep_core_cells"]})
        sat["components"] = []
        for kc in [int(v) for v in a.components.split(",") if v]:
            cbv_k = np.array([tbv * (j + 1) / kc for j in range(kc)])
            acc_k = np.array([(1.0 + 0.5 * j) * acc for j in range(kc)])
            ads_k = np.zeros((kc, nc))
            ads_k[0] = 0.5 * acc
            c0_k = rng.random((kc, nc))
            alone_ms, with_ms, multi_ms = [], [], []
            entry = {"k": kc}
            try:
                for _ in range(a.reps + 1):  # (the first repeat warms up: dropped)
                    sa, ainfo_ = ctx.transport_advance_nl(s0, a.steps, acc, tbv, corey.kind, corey.params, rtol=1e-10,
                                                          raise_on_fail=False)
                    alone = ctx.stats()
                    alone_ms.append(alone["transport_nl_ms"] / max(a.steps, 1))
                    sc, cc, cinfo = ctx.transport_advance_nl_multi(s0, c0_k, a.steps, acc, tbv, cbv_k, corey.kind,
                                                                   corey.params, sorption=ads_k, rtol=1e-10,
                                                                   raise_on_fail=False)
                    both = ctx.stats()
                    with_ms.append(both["transport_nl_ms"] / max(a.steps, 1))
                    cm, minfo = ctx.transport_advance_multi(c0_k, a.steps, acc_k, cbv_k, rtol=1e-10, raise_on_fail=False,
                                                            precond="sweep")
                    multi = ctx.stats()
                    multi_ms.append(multi["transport_advance_ms"] / max(a.steps, 1))
                entry.update({
                    "steps_done": cinfo["steps_done"], "corey_alone_ms_per_step": (min(alone_ms[1:]), float(np.median(alone_ms[1:]))),
                    "corey_with_components_ms_per_step": (min(with_ms[1:]), float(np.median(with_ms[1:]))),
                    "linear_components_ms_per_step": (min(multi_ms[1:]), float(np.median(multi_ms[1:]))),
                    "levels": both["sweep_levels"], "launches_per_step": both["sweep_launches"],
                    "launches_per_step_alone": alone["sweep_launches"], "launches_per_sweep_linear": multi["sweep_launches"],
                    "linear_direct_steps": multi["transport_multi_direct_steps"], "core_cells": both["sweep_core_cells"],
                    "rel_residual_last_step": cinfo["rel_residual"], "max_c_rel_residual_last_step": max(cinfo["c_rel_residual"]),
                    "saturation_bits_equal": bool(sc.tobytes() == sa.tobytes()),
                    "c_min": float(cc.min()), "c_max": float(cc.max())})
            except pa.PorefvError as e:
                entry["error"] = e.message
            sat["components"].append(entry)
        out["saturation"] = sat
        ctx.upwind_assemble(tbv, None, accumulation=acc)  # (the saturation call leaves no system behind)
    if a.saturation and a.adjoint:
        n_obs = 16
        corey = pa.CoreyFractionalFlow(s_wr=0.1, s_nr=0.15, n_w=2.0, n_n=2.0, mu_w=1.0, mu_n=5.0)
        sink = 0.05 * acc * rng.random(nc)
        nl = dict(sink=sink, rtol=1e-10)
        states = np.empty((a.steps + 1, nc))
        states[0] = 0.15 + 0.5 * rng.random(nc)
        obs = np.sort(rng.permutation(nc)[:n_obs])
        loads = rng.standard_normal((a.steps, n_obs))
        entry = {"observation_cells": n_obs}
        try:
            for s_ in range(a.steps):  # the states of the forward run, one step at a time
                states[s_ + 1], ninfo = ctx.transport_advance_nl(states[s_], 1, acc, tbv, corey.kind, corey.params, **nl)
            fwd_ms, adj3_ms, adj7_ms = [], [], []
            for _ in range(a.reps + 1):  # (the first repeat warms up: dropped)
                sn, ninfo = ctx.transport_advance_nl(states[0], a.steps, acc, tbv, corey.kind, corey.params,
                                                     raise_on_fail=False, **nl)
                fwd = ctx.stats()
                fwd_ms.append(fwd["transport_nl_ms"] / max(a.steps, 1))
                g3, i3 = ctx.transport_adjoint_nl(a.steps, acc, tbv, corey.kind, corey.params, loads, states, obs_cells=obs,
                                                  raise_on_fail=False, **nl)
                adj3_ms.append(ctx.stats()["transport_nl_adjoint_ms"] / max(a.steps, 1))
                g7, i7 = ctx.transport_adjoint_nl(a.steps, acc, tbv, corey.kind, corey.params, loads, states, obs_cells=obs,
                                                  want=ctx.NL_ADJOINT_GRADIENTS, raise_on_fail=False, **nl)
                adj = ctx.stats()
                adj7_ms.append(adj["transport_nl_adjoint_ms"] / max(a.steps, 1))
            entry.update({
                "steps_done": i7["steps_done"], "forward_steps_done": ninfo["steps_done"],
                "forward_saturation_ms_per_step": (min(fwd_ms[1:]), float(np.median(fwd_ms[1:]))),
                "adjoint_ms_per_step_s0_source_bc": (min(adj3_ms[1:]), float(np.median(adj3_ms[1:]))),
                "adjoint_ms_per_step_all_seven": (min(adj7_ms[1:]), float(np.median(adj7_ms[1:]))),
                "levels": adj["sweep_levels"], "core_cells": adj["sweep_core_cells"],
                "forward_launches_per_sweep": fwd["sweep_launches"], "adjoint_launches_per_sweep": adj["sweep_launches"],
                "core_iterations": adj["transport_nl_adjoint_core_iterations"],
                "rel_residual_last_step": i7["rel_residual"], "forward_rel_residual_last_step": ninfo["rel_residual"],
                "s_min": float(states.min()), "s_max": float(states.max()),
                "grad_flux_function": g7["flux_function"].tolist(),
                "s0_bits_equal_between_the_two_adjoint_calls": bool(g3["s0"].tobytes() == g7["s0"].tobytes())})
        except pa.PorefvError as e:
            entry["error"] = e.message
        out["saturation_adjoint"] = entry
        ctx.upwind_assemble(tbv, None, accumulation=acc)  # (the calls leave no system behind)
        for kc in [int(v) for v in a.components.split(",") if v]:
            # the same flux, curve, sink and protocol with kc phase-carried components: the forward step of
            # --saturation --components (transport_advance_nl_multi) against its adjoint, alternating
            cbv_k = np.array([tbv * (j + 1) / kc for j in range(kc)])
            ads_k = np.zeros((kc, nc))
            ads_k[0] = 0.3 * acc
            s_st, c_st = np.empty((a.steps + 1, nc)), np.empty((a.steps + 1, kc, nc))
            s_st[0], c_st[0] = states[0], 0.2 + rng.random((kc, nc))
            s_loads, c_loads = rng.standard_normal((a.steps, n_obs)), rng.standard_normal((a.steps, kc, n_obs))
            fw = dict(sorption=ads_k, sink=sink, rtol=1e-10)
            entry = {"k": kc, "observation_cells": n_obs}
            try:
                for s_ in range(a.steps):  # the states of the forward run, one step at a time
                    s_st[s_ + 1], c_st[s_ + 1], cinfo = ctx.transport_advance_nl_multi(
                        s_st[s_], c_st[s_], 1, acc, tbv, cbv_k, corey.kind, corey.params, **fw)
                aj = dict(s_loads=s_loads, c_loads=c_loads, sorption=ads_k, sink=sink, obs_cells=obs, rtol=1e-10,
                          raise_on_fail=False)
                fwd_ms, adj4_ms, adj11_ms = [], [], []
                for _ in range(a.reps + 1):  # (the first repeat warms up: dropped)
                    sc, cc, cinfo = ctx.transport_advance_nl_multi(s_st[0], c_st[0], a.steps, acc, tbv, cbv_k, corey.kind,
                                                                   corey.params, raise_on_fail=False, **fw)
                    fwd = ctx.stats()
                    fwd_ms.append(fwd["transport_nl_ms"] / max(a.steps, 1))
                    g4, i4 = ctx.transport_adjoint_nl_multi(a.steps, acc, tbv, cbv_k, corey.kind, corey.params, s_st, c_st,
                                                            **aj)
                    adj4_ms.append(ctx.stats()["transport_nlc_adjoint_ms"] / max(a.steps, 1))
                    g11, i11 = ctx.transport_adjoint_nl_multi(a.steps, acc, tbv, cbv_k, corey.kind, corey.params, s_st,
                                                              c_st, want=ctx.NLC_ADJOINT_GRADIENTS, **aj)
                    adj = ctx.stats()
                    adj11_ms.append(adj["transport_nlc_adjoint_ms"] / max(a.steps, 1))
                entry.update({
                    "steps_done": i11["steps_done"], "forward_steps_done": cinfo["steps_done"],
                    "forward_ms_per_step": (min(fwd_ms[1:]), float(np.median(fwd_ms[1:])), max(fwd_ms[1:])),
                    "adjoint_ms_per_step_s0_c0_source_c_source": (min(adj4_ms[1:]), float(np.median(adj4_ms[1:])),
                                                                  max(adj4_ms[1:])),
                    "adjoint_ms_per_step_all_eleven": (min(adj11_ms[1:]), float(np.median(adj11_ms[1:])), max(adj11_ms[1:])),
                    "levels": adj["sweep_levels"], "core_cells": adj["sweep_core_cells"],
                    "forward_launches_per_sweep": fwd["sweep_launches"], "adjoint_launches_per_sweep": adj["sweep_launches"],
                    "core_iterations": adj["transport_nlc_adjoint_core_iterations"],
                    "rel_residual_last_step": i11["rel_residual"],
                    "max_c_rel_residual_last_step": max(i11["c_rel_residual"]),
                    "forward_rel_residual_last_step": cinfo["rel_residual"],
                    "grad_flux_function": g11["flux_function"].tolist(),
                    "c0_bits_equal_between_the_two_adjoint_calls": bool(g4["c0"].tobytes() == g11["c0"].tobytes())})
            except pa.PorefvError as e:
                entry["error"] = e.message
            out.setdefault("satcomp_adjoint", []).append(entry)
            ctx.upwind_assemble(tbv, None, accumulation=acc)  # (the calls leave no system behind)
    if a.reactive and a.adjoint:
        kc, n_obs = 4, 16
        acc_k = np.array([(1.0 + 0.5 * j) * acc for j in range(kc)])
        bv_k = np.array([tbv * (j + 1) / kc for j in range(kc)])
        l0, l1, l2, kf, kb = 20.0, 10.0, 2.0, 30.0, 15.0  # the network and the weight of --reactive
        Kr = np.zeros((kc, kc))
        Kr[0, 0], Kr[1, 0], Kr[3, 0] = l0 + kf, -l0, -kf
        Kr[1, 1], Kr[2, 1] = l1, -l1
        Kr[2, 2] = l2
        Kr[3, 3], Kr[0, 3] = kb, -kb
        mobility = np.array([1.0, 1.0, 1.0, 0.0])
        pore_volume = 0.2 * g.cell_volumes
        react = dict(rate_weight=pore_volume, mobility=mobility, rtol=1e-10)
        states = np.empty((a.steps + 1, kc, nc))
        states[0] = rng.random((kc, nc))
        obs = np.sort(rng.permutation(nc)[:n_obs])
        loads = rng.standard_normal((a.steps, kc, n_obs))
        entry = {"k": kc, "observation_cells": n_obs}
        try:
            for s_ in range(a.steps):  # the states of the forward run, one step at a time
                states[s_ + 1], rinfo = ctx.transport_advance_react(states[s_], 1, acc_k, bv_k, Kr, **react)
            fwd_ms, adj3_ms, adj7_ms = [], [], []
            for _ in range(a.reps + 1):  # (the first repeat warms up: dropped)
                cr, rinfo = ctx.transport_advance_react(states[0], a.steps, acc_k, bv_k, Kr, raise_on_fail=False, **react)
                fwd = ctx.stats()
                fwd_ms.append(fwd["transport_react_ms"] / max(a.steps, 1))
                g3, i3 = ctx.transport_adjoint_react(a.steps, acc_k, bv_k, Kr, loads, obs_cells=obs, raise_on_fail=False,
                                                     **react)
                adj3_ms.append(ctx.stats()["transport_react_adjoint_ms"] / max(a.steps, 1))
                g7, i7 = ctx.transport_adjoint_react(a.steps, acc_k, bv_k, Kr, loads, obs_cells=obs, states=states,
                                                     want=ctx.REACT_ADJOINT_GRADIENTS, raise_on_fail=False, **react)
                adj = ctx.stats()
                adj7_ms.append(adj["transport_react_adjoint_ms"] / max(a.steps, 1))
            J = float(np.sum(loads * states[1:][:, :, obs]))
            lin = float(np.sum(g7["c0"] * states[0]) + np.sum(g7["bc_values"] * bv_k))
            entry.update({
                "steps_done": i7["steps_done"], "forward_steps_done": rinfo["steps_done"],
                "forward_reactive_ms_per_step": (min(fwd_ms[1:]), float(np.median(fwd_ms[1:]))),
                "adjoint_ms_per_step_c0_source_bc": (min(adj3_ms[1:]), float(np.median(adj3_ms[1:]))),
                "adjoint_ms_per_step_all_seven": (min(adj7_ms[1:]), float(np.median(adj7_ms[1:]))),
                "levels": adj["sweep_levels"], "core_cells": adj["sweep_core_cells"],
                "forward_launches_per_sweep": fwd["sweep_launches"], "adjoint_launches_per_sweep": adj["sweep_launches"],
                "core_iterations": adj["transport_react_adjoint_core_iterations"],
                "max_rel_residual_last_step": max(i7["rel_residual"]),
                "identity_J_minus_products_relative": abs(J - lin) / max(abs(J), 1e-300),
                "grad_rate_matrix": g7["rate_matrix"].tolist(),
                "c0_bits_equal_between_the_two_adjoint_calls": bool(g3["c0"].tobytes() == g7["c0"].tobytes())})
        except pa.PorefvError as e:
            entry["error"] = e.message
        out["reactive_adjoint"] = entry
        ctx.upwind_assemble(tbv, None, accumulation=acc)  # (the calls leave no system behind)
    if a.reactive and not a.adjoint:
        kc = 4
        acc_k = np.array([(1.0 + 0.5 * j) * acc for j in range(kc)])
        bv_k = np.array([tbv * (j + 1) / kc for j in range(kc)])
        c0_k = rng.random((kc, nc))
        l0, l1, l2, kf, kb = 20.0, 10.0, 2.0, 30.0, 15.0  # rates per unit time; dt = 0.5 / n
        Kr = np.zeros((kc, kc))
        Kr[0, 0], Kr[1, 0], Kr[3, 0] = l0 + kf, -l0, -kf
        Kr[1, 1], Kr[2, 1] = l1, -l1
        Kr[2, 2] = l2
        Kr[3, 3], Kr[0, 3] = kb, -kb
        mobility = np.array([1.0, 1.0, 1.0, 0.0])
        pore_volume = 0.2 * g.cell_volumes
        lin_ms, react_ms = [], []
        entry = {"k": kc}
        try:
            for _ in range(a.reps + 1):  # (the first repeat builds the order and warms up: dropped)
                cm, minfo = ctx.transport_advance_multi(c0_k, a.steps, acc_k, bv_k, rtol=1e-10, raise_on_fail=False,
                                                        precond="sweep")
                multi = ctx.stats()
                lin_ms.append(multi["transport_advance_ms"] / max(a.steps, 1))
                cr, rinfo = ctx.transport_advance_react(c0_k, a.steps, acc_k, bv_k, Kr, rate_weight=pore_volume,
                                                        mobility=mobility, rtol=1e-10, raise_on_fail=False)
                react = ctx.stats()
                react_ms.append(react["transport_react_ms"] / max(a.steps, 1))
            entry.update({
                "steps_done": rinfo["steps_done"], "linear_steps_done": minfo["steps_done"],
                "linear_components_ms_per_step": (min(lin_ms[1:]), float(np.median(lin_ms[1:]))),
                "reactive_ms_per_step": (min(react_ms[1:]), float(np.median(react_ms[1:]))),
                "levels": react["sweep_levels"], "core_cells": react["sweep_core_cells"],
                "launches_per_step": react["sweep_launches"], "launches_per_sweep_linear": multi["sweep_launches"],
                "linear_direct_steps": multi["transport_multi_direct_steps"],
                "core_iterations": react["transport_react_core_iterations"],
                "max_rel_residual_last_step": max(rinfo["rel_residual"]),
                "c_min": float(cr.min()), "c_max": float(cr.max())})
        except pa.PorefvError as e:
            entry["error"] = e.message
        out["reactive"] = entry
        ctx.upwind_assemble(tbv, None, accumulation=acc)  # (the reactive call leaves no system behind)
    if a.sorbing:
        kc = 4
        four = [(_lib.ISOTHERM_FREUNDLICH, (1.0, 0.5)), (_lib.ISOTHERM_FREUNDLICH, (0.8, 0.7)),
                (_lib.ISOTHERM_LANGMUIR, (2.0, 3.0)), (_lib.ISOTHERM_LINEAR, (1.0, 0.0))]

        def problem(kk):
            iso = [four[j % 4] for j in range(kk)]
            acc_k = np.array([(1.0 + 0.5 * (j % 4)) * acc for j in range(kk)])
            bv_k = np.array([tbv * (j % 4 + 1) / 4 for j in range(kk)])
            state = np.random.default_rng(7).random((kk, nc))
            return [m for m, _ in iso], np.array([p for _, p in iso]), acc_k, bv_k, 0.5 * acc_k, state

        kinds, par, acc_k, bv_k, cap_k, c0_k = problem(kc)
        lin_ms, sorb_ms, fold_ms = [], [], []
        entry = {"k": kc}
        try:
            for _ in range(a.reps + 1):  # (the first repeat builds the order and warms up: dropped)
                cm, minfo = ctx.transport_advance_multi(c0_k, a.steps, acc_k, bv_k, rtol=1e-10, raise_on_fail=False,
                                                        precond="sweep")
                multi = ctx.stats()
                lin_ms.append(multi["transport_advance_ms"] / max(a.steps, 1))
                cs, sinfo = ctx.transport_advance_sorb(c0_k, a.steps, acc_k, bv_k, kinds, par, capacity=cap_k, rtol=1e-10,
                                                       raise_on_fail=False)
                sorb = ctx.stats()
                sorb_ms.append(sorb["transport_sorb_ms"] / max(a.steps, 1))
                cf, finfo = ctx.transport_advance_sorb(c0_k, a.steps, acc_k, bv_k, [_lib.ISOTHERM_LINEAR] * kc,
                                                       np.array([[1.0, 0.0]] * kc), capacity=cap_k, rtol=1e-10,
                                                       raise_on_fail=False)
                fold_ms.append(ctx.stats()["transport_sorb_ms"] / max(a.steps, 1))
            entry.update({
                "steps_done": sinfo["steps_done"], "linear_steps_done": minfo["steps_done"],
                "all_linear_steps_done": finfo["steps_done"],
                "linear_components_ms_per_step": (min(lin_ms[1:]), float(np.median(lin_ms[1:]))),
                "sorbing_ms_per_step": (min(sorb_ms[1:]), float(np.median(sorb_ms[1:]))),
                "sorbing_all_linear_ms_per_step": (min(fold_ms[1:]), float(np.median(fold_ms[1:]))),
                "levels": sorb["sweep_levels"], "core_cells": sorb["sweep_core_cells"],
                "launches_per_step": sorb["sweep_launches"], "launches_per_sweep_linear": multi["sweep_launches"],
                "linear_direct_steps": multi["transport_multi_direct_steps"],
                "core_iterations": sorb["transport_sorb_core_iterations"],
                "max_rel_residual_last_step": max(sinfo["rel_residual"]),
                "c_min": float(cs.min()), "c_max": float(cs.max())})
            for kk in [int(t) for t in a.components.split(",") if t]:
                kinds, par, acc_k, bv_k, cap_k, c0_k = problem(kk)
                ms = []
                for _ in range(a.reps + 1):
                    cs, sinfo = ctx.transport_advance_sorb(c0_k, a.steps, acc_k, bv_k, kinds, par, capacity=cap_k,
                                                           rtol=1e-10, raise_on_fail=False)
                    ms.append(ctx.stats()["transport_sorb_ms"] / max(a.steps, 1))
                entry[f"k{kk}_sorbing_ms_per_step"] = (min(ms[1:]), float(np.median(ms[1:])))
                entry[f"k{kk}_steps_done"] = sinfo["steps_done"]
        except pa.PorefvError as e:
            entry["error"] = e.message
        out["sorbing"] = entry
        ctx.upwind_assemble(tbv, None, accumulation=acc)  # (the sorbing call leaves no system behind)
    if a.adjoint and not a.reactive and not a.saturation:
        kc, n_obs = 4, 16
        acc_k = np.array([(1.0 + 0.5 * j) * acc for j in range(kc)])
        bv_k = np.array([tbv * (j + 1) / kc for j in range(kc)])
        states = np.empty((a.steps + 1, kc, nc))
        states[0] = rng.random((kc, nc))
        obs = np.sort(rng.permutation(nc)[:n_obs])
        loads = rng.standard_normal((a.steps, kc, n_obs))
        entry = {"k": kc, "observation_cells": n_obs}
        try:
            for s_ in range(a.steps):  # the states of the forward run, one step at a time
                states[s_ + 1], minfo = ctx.transport_advance_multi(states[s_], 1, acc_k, bv_k, rtol=1e-10, precond="sweep")
            fwd_ms, adj3_ms, adj5_ms = [], [], []
            for _ in range(a.reps + 1):  # (the first repeat warms up: dropped)
                cm, minfo = ctx.transport_advance_multi(states[0], a.steps, acc_k, bv_k, rtol=1e-10, raise_on_fail=False,
                                                        precond="sweep")
                multi = ctx.stats()
                fwd_ms.append(multi["transport_advance_ms"] / max(a.steps, 1))
                g3, i3 = ctx.transport_adjoint_multi(a.steps, acc_k, bv_k, loads, obs_cells=obs, rtol=1e-10,
                                                     raise_on_fail=False)
                adj3_ms.append(ctx.stats()["transport_adjoint_ms"] / max(a.steps, 1))
                g5, i5 = ctx.transport_adjoint_multi(a.steps, acc_k, bv_k, loads, obs_cells=obs, states=states,
                                                     want=ctx.ADJOINT_GRADIENTS, rtol=1e-10, raise_on_fail=False)
                adj = ctx.stats()
                adj5_ms.append(adj["transport_adjoint_ms"] / max(a.steps, 1))
            J = float(np.sum(loads * states[1:][:, :, obs]))
            lin = float(np.sum(g5["c0"] * states[0]) + np.sum(g5["bc_values"] * bv_k))
            entry.update({
                "steps_done": i5["steps_done"], "forward_steps_done": minfo["steps_done"],
                "forward_ms_per_step": (min(fwd_ms[1:]), float(np.median(fwd_ms[1:]))),
                "adjoint_ms_per_step_c0_source_bc": (min(adj3_ms[1:]), float(np.median(adj3_ms[1:]))),
                "adjoint_ms_per_step_all_five": (min(adj5_ms[1:]), float(np.median(adj5_ms[1:]))),
                "levels": adj["sweep_levels"], "core_cells": adj["sweep_core_cells"],
                # per step: the sweep, then forward rhs + 2 norms kernels; adjoint rhs + 2 norms kernels (+ one
                # interleave of the slab, grad_bc_values and grad_flux with all five)
                "forward_launches_per_step": {"sweep": multi["sweep_launches"], "other": 3},
                "adjoint_launches_per_step": {"sweep": adj["sweep_launches"], "other_c0_source_bc": 4, "other_all_five": 6},
                "core_iterations": adj["transport_adjoint_core_iterations"],
                "max_rel_residual_last_step": max(i5["rel_residual"]),
                "identity_J_minus_products_relative": abs(J - lin) / max(abs(J), 1e-300),
                "c0_bits_equal_between_the_two_adjoint_calls": bool(g3["c0"].tobytes() == g5["c0"].tobytes())})
        except pa.PorefvError as e:
            entry["error"] = e.message
        out["adjoint"] = entry
        ctx.upwind_assemble(tbv, None, accumulation=acc)  # (the adjoint call leaves no system behind)
    # bytes each kernel has to move at least ("Upwind advection"): the fraction of a stream rate follows
    nnz_flux = ctx.matrix_info(_lib.MAT_FLUX)[2]
    nnz_bound = ctx.matrix_info(_lib.MAT_BOUND_FLUX)[2]
    nnz_T = ctx.matrix_info(_lib.MAT_TRANSPORT_SYSTEM)[2]
    ncf = ctx.ncf
    out["min_bytes"] = {
        "face_flux": 12 * (nnz_flux + nnz_bound) + 8 * (nf + nc) + 8 * nf,
        "upwind_discretize": nf * (8 + 8 + 8 + 1 + 4 + 12 + 16) + 3 * 4 * nf + 12 * nf,
        "transport_assemble": 12 * nnz_T + ncf * (4 + 1 + 1 + 4 + 8) + 8 * 4 * nc,
    }
    if not a.no_host:
        flux, bflux = ctx.matrix(_lib.MAT_FLUX), ctx.matrix(_lib.MAT_BOUND_FLUX)
        t0 = time.perf_counter()
        qh = flux @ p + bflux @ fbv
        t1 = time.perf_counter()
        cf = sps.csc_matrix(g.cell_faces)
        fi, ci, sg = sps.find(cf)
        side = -np.ones((2, nf), dtype=np.int64)
        side[0, fi[sg > 0]] = ci[sg > 0]
        side[1, fi[sg < 0]] = ci[sg < 0]
        pos = np.sign(qh) >= 0
        up = np.where(pos, side[0], side[1])
        isd = np.zeros(nf, dtype=bool)
        isd[bf] = True
        dirin = isd & (up < 0)
        f = np.flatnonzero(~dirin)
        U = sps.coo_matrix((np.ones(f.size), (f, up[f])), shape=(nf, nc)).tocsr()
        fd = np.flatnonzero(dirin)
        D = sps.coo_matrix((np.ones(fd.size), (fd, fd)), shape=(nf, nf)).tocsr()
        t2 = time.perf_counter()
        div = cf.T.tocsr()
        Q = sps.diags(qh)
        Ah = (div @ Q @ U + sps.diags(acc)).tocsr()
        bh = div @ ((D @ Q) @ tbv)
        t3 = time.perf_counter()
        out["host_ms"] = {"face_flux": 1e3 * (t1 - t0), "upwind_discretize": 1e3 * (t2 - t1),
                          "assemble": 1e3 * (t3 - t2)}
        # the host step: the same Jacobi-BiCGStab through scipy on the host matrix
        import scipy.sparse.linalg as spla

        Mj = spla.LinearOperator((nc, nc), matvec=lambda x: x / Ah.diagonal())
        ch = c0.copy()
        hsteps = min(a.steps, 3)
        # every step is judged by its TRUE relative residual ||r - M c|| / ||r|| against the host matrix, for the host
        # solve and for the device solve advanced one step at a time from the same state
        flags, res_h, res_d, gap = [], [], [], []
        cd = c0.copy()
        t_host = 0.0
        for _ in range(hsteps):
            rh = acc * ch - bh
            t4 = time.perf_counter()
            ch_new, flag = spla.bicgstab(Ah, rh, x0=ch, rtol=1e-10, M=Mj, maxiter=5000)
            t_host += time.perf_counter() - t4
            flags.append(int(flag))
            res_h.append(float(np.linalg.norm(rh - Ah @ ch_new) / np.linalg.norm(rh)))
            ch = ch_new
            rd = acc * cd - bh
            cd, _ = ctx.transport_advance(cd, 1, rtol=1e-10, raise_on_fail=False)
            res_d.append(float(np.linalg.norm(rd - Ah @ cd) / np.linalg.norm(rd)))
            gap.append(float(np.abs(cd - ch).max()))
        out["host_ms"]["step"] = 1e3 * t_host / hsteps
        out["host_bicgstab_flags"] = flags  # scipy: 0 converged, > 0 iterations exhausted, < 0 breakdown
        out["true_rel_residual_host"] = res_h
        out["true_rel_residual_device"] = res_d
        out["device_vs_host_max_diff_per_step"] = gap
        out["gmres_retries_last_advance"] = ctx.stats()["transport_gmres_retries"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
