"""Time of the adjoint of the flow solve next to the forward flow solve on the same handle and grid (6 * n^3 perturbed
tetrahedra; n = 35: 257 250 cells), with the same method, rtol and preconditioner:

    discretize -> [ assemble + solve (the yardstick, unchanged code)  |  flow_adjoint ] alternating, --reps times

Device times are HIP-event times from pfv_stats (solve_ms of the forward solve; flow_adjoint_map_ms / _products_ms /
_solve_ms / _gradient_ms of the adjoint), the call times are a host clock around calls that end in a device
synchronise.  The first repeat (which builds the column maps and loads the code objects) is reported apart and dropped
from best / median.  With --scheme mpfa the adjoint also asks for "permeability_exact": exact_ms is the kernel pair of
the exact gradient (the interaction-region pass and the cell sum, flow_adjoint_exact_ms), to be read next to node_ms --
the interaction-region kernel of the discretize call on the same grid, reported once -- and gradient_ms, the face and
cell kernels of the two-point grad_perm.  Prints one JSON line.  A measurement, not a test: no thresholds.

    python tools/bench_flow_adjoint.py [--n-side 35] [--scheme mpfa|tpfa] [--reps 6] [--rtol 1e-10] [--precond amg]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-side", type=int, default=35)
    ap.add_argument("--scheme", choices=["mpfa", "tpfa"], default="mpfa")
    ap.add_argument("--reps", type=int, default=6)
    ap.add_argument("--rtol", type=float, default=1e-10)
    ap.add_argument("--precond", default="amg")
    ap.add_argument("--method", default="")
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
    bv = np.zeros(nf)
    bv[bf] = g.face_centers[:, bf].sum(axis=0)
    data = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": bc, "bc_values": bv})
    flow = (pa.Mpfa if a.scheme == "mpfa" else pa.Tpfa)("flow", library=lib)
    method = a.method or ("bicgstab" if a.scheme == "mpfa" else "cg")
    flow.discretize(g, data)
    ctx = flow.context(g)
    st0 = ctx.stats()
    discretize = {"node_ms": st0["node_ms"], "discretize_ms": st0["discretize_ms"]}
    want = ("permeability", "bc_values", "source") + (("permeability_exact",) if a.scheme == "mpfa" else ())
    source = g.cell_volumes * rng.standard_normal(nc)
    gq, gp = rng.standard_normal(nf), rng.standard_normal(nc)
    kw = dict(method=method, rtol=a.rtol, precond=a.precond)
    fwd, adj = [], []
    p = None
    for _ in range(a.reps):
        t0 = time.perf_counter()
        p, info = flow.solve(g, data, source=source, **kw)
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e3
        st = ctx.stats()
        fwd.append({"call_ms": wall, "solve_ms": st["solve_ms"], "assemble_ms": st["assemble_ms"],
                    "amg_setup_ms": st["amg_setup_ms"], "iterations": info["iterations"]})
        t0 = time.perf_counter()
        _, info = flow.adjoint_flow(g, data, p, grad_flux=gq, grad_pressure=gp, want=want, **kw)
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e3
        st = ctx.stats()
        adj.append({"call_ms": wall, "map_ms": st["flow_adjoint_map_ms"], "products_ms": st["flow_adjoint_products_ms"],
                    "solve_ms": st["flow_adjoint_solve_ms"], "gradient_ms": st["flow_adjoint_gradient_ms"],
                    "exact_ms": st["flow_adjoint_exact_ms"], "exact_map_ms": st["flow_adjoint_exact_map_ms"],
                    "amg_setup_ms": st["amg_setup_ms"], "iterations": info["iterations"],
                    "map_builds": st["flow_adjoint_map_builds"]})

    def summary(rows):
        rest = rows[1:] if len(rows) > 1 else rows
        keys = [m for m in rows[0] if m.endswith("_ms")]
        return {"first": rows[0], "best": {m: min(r[m] for r in rest) for m in keys},
                "median": {m: float(np.median([r[m] for r in rest])) for m in keys},
                "iterations": sorted({r["iterations"] for r in rows}), "repeats_kept": len(rest)}

    print(json.dumps({"scheme": a.scheme, "cells": int(nc), "faces": int(nf), "flux_nnz": int(ctx.matrix_info(0)[2]),
                      "method": method, "rtol": a.rtol, "precond": a.precond, "device_build": lib is None,
                      "discretize": discretize, "forward": summary(fwd), "adjoint": summary(adj)}))


if __name__ == "__main__":
    main()
