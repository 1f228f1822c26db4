"""Time of the adjoint of the advection-diffusion step next to the forward run on the same handle and grid (6 * n^3
perturbed tetrahedra; n = 35: 257 250 cells), with the same method, rtol and preconditioner:

    discretize -> [ advance of N steps (the yardstick, unchanged code)  |  adjoint of N steps ] alternating, --reps times

Both calls assemble the system first, as the class does.  Device times are HIP-event times from pfv_stats
(advdiff_advance_ms of the forward run; advdiff_adjoint_ms and advdiff_adjoint_accumulate_ms of the adjoint), the call
times are a host clock around calls that end in a device synchronise.  The first repeat (which builds the column map
and the transposed positions and loads the code objects) is reported apart and dropped from best / median.  Prints one
JSON line.  A measurement, not a test: no thresholds.

--exact: every repeat also runs the adjoint with "conductivity_exact" added to ``want`` (pfv_advdiff_adjoint_exact), once
per value of --exact-batch (0: the library's default), and reports advdiff_adjoint_exact_ms (the interaction-region
passes and the cell sum) and advdiff_adjoint_exact_passes beside the fields of the call without the key.

    python tools/bench_advdiff_adjoint.py [--n-side 35] [--steps 8] [--scheme mpfa|tpfa] [--reps 6] [--rtol 1e-10]
                                          [--precond amg] [--want all|default] [--exact [--exact-batch B [B ...]]]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import porepy_amd as pa  # noqa: E402

KW = "transport"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-side", type=int, default=35)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--scheme", choices=["mpfa", "tpfa"], default="mpfa")
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--precond", default="amg")
    ap.add_argument("--method", default="bicgstab")
    ap.add_argument("--want", choices=["all", "default"], default="all")
    ap.add_argument("--exact", action="store_true", help='also time the call with "conductivity_exact"')
    ap.add_argument("--exact-batch", type=int, nargs="+", default=[0], help="steps per region pass (0: the default)")
    ap.add_argument("--emulation", action="store_true", help="run on the host-emulation build (plumbing check)")
    a = ap.parse_args()
    lib = None
    if a.emulation:
        from tests import _parity as P

        lib = P.emulation_library()
    n, N = a.n_side, a.steps
    g = pa.StructuredTetrahedralGrid([n, n, n], [1.0, 1.0, 1.0])
    g.compute_geometry()
    g = pa.perturb_interior_nodes(g, 0.2 / n)
    nc, nf = g.num_cells, g.num_faces
    rng = np.random.default_rng(0)
    k = 1 + rng.random(nc)
    K = pa.SecondOrderTensor(kxx=k, kyy=1.5 * k, kzz=0.7 * k, kxy=0.1 * k)
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, list(np.array(["dir", "neu", "dir"])[np.arange(bf.size) % 3]))
    bv = np.zeros(nf)
    bv[bf] = np.where(bc.is_dir[bf], 0.25 + rng.random(bf.size), 0.05 * (rng.random(bf.size) - 0.5) * g.face_areas[bf])
    q = pa.Upwind(KW).darcy_flux(g, [0.6, -0.3, 0.45])
    data = pa.initialize_data({}, KW, {"second_order_tensor": K, "bc": bc, "bc_values": bv, "darcy_flux": q,
                                       "flux_scale": 1.7})
    vol = np.asarray(g.cell_volumes, dtype=float)
    acc = (0.2 + 0.3 * rng.random(nc)) * vol / 0.05
    c0, src = rng.random(nc), 0.1 * (rng.random(nc) - 0.5) * vol
    loads = rng.standard_normal((N, nc))
    ad = pa.AdvectionDiffusion(KW, scheme=a.scheme, library=lib)
    ad.discretize(g, data)
    ctx = ad.context(g)
    kw = dict(method=a.method, rtol=a.rtol, precond=a.precond)
    want = ctx.ADVDIFF_ADJOINT_GRADIENTS if a.want == "all" else ("c0", "source", "bc_values")
    _, info, states = ad.advance(g, data, c0, N, acc, source=src, return_states=True, **kw)
    assert info["steps_done"] == N
    fwd, adj = [], []
    exact = {b: [] for b in (a.exact_batch if a.exact else [])}

    def adjoint_row(want_, **more):
        t0 = time.perf_counter()
        _, info = ad.adjoint(g, data, N, acc, loads, states, source=src, want=want_, **kw, **more)
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e3
        st = ctx.stats()
        return {"call_ms": wall, "assemble_ms": st["advdiff_assemble_ms"], "adjoint_ms": st["advdiff_adjoint_ms"],
                "accumulate_ms": st["advdiff_adjoint_accumulate_ms"], "amg_setup_ms": st["amg_setup_ms"],
                "exact_ms": st["advdiff_adjoint_exact_ms"], "exact_passes": st["advdiff_adjoint_exact_passes"],
                "exact_batch": st["advdiff_adjoint_exact_batch"], "iterations": st["advdiff_adjoint_iterations"],
                "fallbacks": st["advdiff_adjoint_precond_fallbacks"] + st["advdiff_adjoint_gmres_retries"],
                "steps": info["steps_done"], "map_builds": st["flow_adjoint_map_builds"]}

    for _ in range(a.reps):
        t0 = time.perf_counter()
        _, info = ad.advance(g, data, c0, N, acc, source=src, **kw)
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e3
        st = ctx.stats()
        fwd.append({"call_ms": wall, "assemble_ms": st["advdiff_assemble_ms"], "advance_ms": st["advdiff_advance_ms"],
                    "amg_setup_ms": st["amg_setup_ms"], "iterations": st["advdiff_iterations"],
                    "fallbacks": st["advdiff_precond_fallbacks"] + st["advdiff_gmres_retries"],
                    "steps": info["steps_done"]})
        adj.append(adjoint_row(want))
        for b in exact:
            exact[b].append(adjoint_row(tuple(want) + ctx.ADVDIFF_ADJOINT_EXACT, exact_batch=b))

    def summary(rows):
        rest = rows[1:] if len(rows) > 1 else rows
        keys = [m for m in rows[0] if m.endswith("_ms")]
        return {"first": rows[0], "best": {m: min(r[m] for r in rest) for m in keys},
                "median": {m: float(np.median([r[m] for r in rest])) for m in keys},
                "worst": {m: max(r[m] for r in rest) for m in keys},
                "exact_passes": sorted({r.get("exact_passes", 0) for r in rows}),
                "exact_batch": sorted({r.get("exact_batch", 0) for r in rows}),
                "iterations": sorted({r["iterations"] for r in rows}), "fallbacks": sorted({r["fallbacks"] for r in rows}),
                "steps": sorted({r["steps"] for r in rows}), "repeats_kept": len(rest)}

    F, A = summary(fwd), summary(adj)
    print(json.dumps({"scheme": a.scheme, "cells": int(nc), "faces": int(nf), "steps": N, "method": a.method,
                      "rtol": a.rtol, "precond": a.precond, "want": list(want), "device_build": lib is None,
                      "forward": F, "adjoint": A,
                      "adjoint_exact": {str(b): summary(rows) for b, rows in exact.items()},
                      "adjoint_over_forward_call_median": A["median"]["call_ms"] / F["median"]["call_ms"],
                      "adjoint_over_forward_device_median": A["median"]["adjoint_ms"] / F["median"]["advance_ms"]}))


if __name__ == "__main__":
    main()
