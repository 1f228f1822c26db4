"""Times of the advection-diffusion step on structured tetrahedra [n]^3 (n = 32: 196 608 cells, MPFA), in one process:

  (a) the fused refresh for a changed flux (update_flux)
  (b) the same change composed through the generic sparse algebra -- upwind system of the new flux, DeviceCsr sum with
      the diffusion handle's system and the diagonal, then as_system
      both as wall clock around synchronised calls from the same host arrays, median after warm-up (the composition
      spans many library calls, so one pair of device events cannot bracket it); for (a) also the HIP-event time of
      its kernels alone (pfv_stats.advdiff_assemble_ms)
  (c) ms and iterations per implicit Euler step of ``advance`` with AMG, with Jacobi and with the flow-ordered sweep at
      cell Peclet 0.05 and 5
  and the stream triad rate of the device (pfv_time_kernel) next to the refresh's algorithmic bytes.

Prints a small report.  A measurement, not a test: no thresholds.

    python tools/advdiff_step.py [--n-side 32] [--steps 5] [--reps 7] [--emulation]
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sps

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import porepy_amd as pa  # noqa: E402
from porepy_amd import _lib  # noqa: E402

KW = "transport"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-side", type=int, default=32)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--emulation", action="store_true", help="run on the host-emulation build (plumbing check)")
    a = ap.parse_args()
    lib = None
    if a.emulation:
        from tests import _parity as P

        lib = P.emulation_library()
    n = a.n_side
    g = pa.StructuredTetrahedralGrid([n, n, n], [1.0, 1.0, 1.0])
    g.compute_geometry()
    nc, nf = g.num_cells, g.num_faces
    rng = np.random.default_rng(0)
    vel = np.array([0.6, -0.3, 0.45])
    q = pa.Upwind(KW).darcy_flux(g, list(vel))
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)
    bv = np.zeros(nf)
    bv[bf] = rng.random(bf.size)
    c0 = rng.random(nc)
    acc = np.asarray(g.cell_volumes) / 0.5
    print(f"structured tetrahedra [{n}]^3: {nc} cells, {nf} faces")
    for pe in (0.05, 5.0):
        D = float(np.linalg.norm(vel)) / n / pe
        k = D * (1 + rng.random(nc))
        K = pa.SecondOrderTensor(kxx=k, kyy=1.5 * k, kzz=0.7 * k, kxy=0.1 * k)
        par = {"second_order_tensor": K, "bc": bc, "bc_values": bv, "darcy_flux": q}
        data = pa.initialize_data({}, KW, par)
        ad = pa.AdvectionDiffusion(KW, library=lib)
        ad.discretize(g, data)
        ctx = ad.context(g)
        ad._assemble(g, data, acc, c0)
        nnz = ctx.matrix_info(_lib.MAT_ADVDIFF_SYSTEM)[2]
        if pe == 0.05:
            # (a) a changed flux on the same discretization: the refresh.  Wall clock around synchronised calls, as
            # for (b), from the same host arrays; the HIP-event time of the kernels alone rides along
            ts, tw = [], []
            for r in range(a.reps + 2):
                data[pa.PARAMETERS][KW]["darcy_flux"] = q * (1.0 + 0.01 * r)
                ctx.sync()
                t0 = time.perf_counter()
                ad.update_flux(g, data, acc, c0)
                ctx.sync()
                tw.append(1e3 * (time.perf_counter() - t0))
                ts.append(ctx.stats()["advdiff_assemble_ms"])
            t_a, t_aw = float(np.median(ts[2:])), float(np.median(tw[2:]))
            data[pa.PARAMETERS][KW]["darcy_flux"] = q
            # (b) the same change through the sparse algebra, two handles: the upwind system of the new flux (same signs:
            # no new upwind discretization), the sum with the diffusion system and the diagonal, as_system
            up = pa.Upwind(KW, library=lib)
            udata = pa.initialize_data({}, KW, {"darcy_flux": q, "bc": bc, "bc_values": bv})
            up.discretize(g, udata)
            uctx = up.context(g)
            ad.diffusion.assemble_matrix_rhs(g, data)
            dacc = pa.DeviceCsr.from_scipy(sps.diags(acc).tocsr(), uctx)
            dD = pa.DeviceCsr.from_discretization(ctx, _lib.MAT_SYSTEM, uctx)
            rhs = acc * c0
            tb = []
            for r in range(a.reps + 2):
                qr = q * (1.0 + 0.01 * r)
                uctx.sync()
                ctx.sync()
                t0 = time.perf_counter()
                uctx.upwind_assemble(bv, qr)
                dA = pa.DeviceCsr.from_discretization(uctx, _lib.MAT_TRANSPORT_SYSTEM)
                dS = dA + dD + dacc
                dS.as_system(rhs)
                uctx.sync()
                tb.append(1e3 * (time.perf_counter() - t0))
            t_b = float(np.median(tb[2:]))
            bytes_alg = 16.0 * nnz
            print(f"(a) fused refresh {t_aw:.3f} ms wall clock ({t_a:.4f} ms in its kernels, HIP events)   "
                  f"(b) composed through DeviceCsr {t_b:.3f} ms wall clock   nnz(pat_A) = {nnz}")
            triad_ms = ctx.time_kernel(4, 5)  # a = b + s c on 3 x 2^27 doubles: 3 * 2^30 bytes per launch
            rate = 3.0 * 2 ** 30 / triad_ms / 1e6
            print(f"    algorithmic bytes 16 nnz = {bytes_alg / 1e6:.2f} MB -> {bytes_alg / t_a / 1e6:.1f} GB/s = "
                  f"{100 * bytes_alg / t_a / 1e6 / rate:.0f} % of the measured stream triad rate {rate:.0f} GB/s")
            ad._assemble(g, data, acc, c0)
        # (c) the step
        for precond in ("amg", "jacobi", "sweep"):
            ad.advance(g, data, c0, 1, acc, precond=precond, rtol=1e-10, raise_on_fail=False)  # warm-up (AMG setup)
            _, info = ad.advance(g, data, c0, a.steps, acc, precond=precond, rtol=1e-10, raise_on_fail=False)
            st = ctx.stats()
            print(f"(c) Peclet {pe:g}, {precond:6s}: {st['advdiff_advance_ms'] / max(info['steps_done'], 1):8.3f} ms/step, "
                  f"{st['advdiff_iterations'] / max(info['steps_done'], 1):6.1f} iterations/step, "
                  f"{info['steps_done']}/{a.steps} steps, {st['advdiff_precond_fallbacks']} fallbacks"
                  + (f", {st['sweep_levels']} levels, {st['sweep_launches']} launches per sweep" if precond == "sweep" else ""))


if __name__ == "__main__":
    main()
