"""configs[3] (MPSA, perturbed structured tetrahedra, rollers + top traction) solved with precond="amg" and with
precond="amg_rbm" (aggregation AMG carrying the rigid-body modes, PFV_PRECOND_AMG_NNS): iterations, setup and solve
times, operator complexity, levels and kernel launches per iteration, one JSON line per preconditioner.

    python tools/amg_nns_bench.py [--n 44] [--rtol 1e-13] [--solves 3] [--only amg|amg_rbm]

The first solve of each preconditioner builds its hierarchy (setup_ms, first_solve_ms includes it); the following
solves on the re-assembled, unchanged values keep it (solve_ms: the Krylov loop alone).
For a kernel table run one solve of one preconditioner under rocprofv3 --kernel-trace --stats (--only, --solves 1)."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import porepy_amd as pa  # noqa: E402


def system(n):
    g = pa.StructuredTetrahedralGrid([n, n, n], [1.0, 1.0, 1.0])
    g.compute_geometry()
    g = pa.perturb_interior_nodes(g, 0.2 / n)
    nc, nf = g.num_cells, g.num_faces
    C = pa.FourthOrderTensor(np.ones(nc), np.ones(nc))
    bc = pa.BoundaryConditionVectorial(g)
    bf = g.get_all_boundary_faces()
    fc = g.face_centers
    for axis in range(3):
        roll = bf[fc[axis, bf] < 1e-9]
        bc.is_dir[axis, roll] = True
        bc.is_neu[axis, roll] = False
    bv = np.zeros((3, nf))
    top = bf[fc[2, bf] > 1 - 1e-9]
    bv[2, top] = -g.face_areas[top]
    ctx = pa.Context(0)
    ctx.set_grid(pa.grid_to_raw(g))
    ctx.mpsa_set_params(C.values, g.cell_volumes, bc.is_dir, bc.is_neu, 1.0 / 3.0)
    ctx.mpsa_discretize(rebuild_topology=False)
    return g, ctx, bv.ravel("F")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=44)
    ap.add_argument("--rtol", type=float, default=1e-13)
    ap.add_argument("--solves", type=int, default=3)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    g, ctx, bvf = system(args.n)
    nc = g.num_cells
    cc = g.cell_centers
    exact = np.vstack((0.25 * cc[0] / 2.5, 0.25 * cc[1] / 2.5, -cc[2] / 2.5))
    for precond in ([args.only] if args.only else ["amg", "amg_rbm"]):
        rows = []
        for _ in range(args.solves):
            ctx.mpsa_assemble(bvf, None)
            u, info = ctx.solve("bicgstab", rtol=args.rtol, maxit=50000, n=3 * nc, raise_on_fail=False, precond=precond)
            st = ctx.stats()
            rows.append((info, st))
        info, st = rows[-1]
        it = max(1, info["iterations"])
        err = float(np.abs(u.reshape(3, -1, order="F") - exact).max())
        print(json.dumps({
            "precond": precond, "cells": nc, "unknowns": 3 * nc, "rtol": args.rtol,
            "iterations": info["iterations"], "converged": info["converged"],
            "rel_residual": info["rel_residual"],
            # the first solve builds the hierarchy; the later ones (same values) keep it
            "setup_ms": round(rows[0][1]["amg_setup_ms"], 3), "first_solve_ms": round(rows[0][0]["solve_ms"], 3),
            "solve_ms": [round(r[0]["solve_ms"], 3) for r in rows[1:]],
            "operator_complexity": round(st["amg_operator_complexity"], 4), "levels": st["amg_levels"],
            "coarsest_rows": st["amg_coarsest_rows"], "modes": st["amg_nns_modes"] if precond != "amg" else 0,
            "setup_launches": rows[0][1]["amg_setup_launches"], "solve_launches": st["solve_launches"],
            "launches_per_iteration": round(st["solve_launches"] / it, 1), "max_error_vs_exact": err,
        }), flush=True)


if __name__ == "__main__":
    main()
