#!/usr/bin/env python
"""bench.py — cells/sec of MPFA assemble + solve on synthetic 3-D simplex box grids.

One "step" = one pass of the hot path over one grid already resident in HBM:
  sub-cell topology + CSR symbolic phase + interaction-region kernel + face kernel
  (= what one ``Mpfa.discretize`` call of the reference does), ``A = div @ flux`` and the
  right-hand side, then the preconditioned BiCGStab solve to rtol (aggregation-AMG cycle by default).
Default workload (N = 1): BASELINE.json configs[2] — ~2 M tetrahedra, perturbed nodes,
full-tensor anisotropic permeability — the grid the north-star target is quoted on.

Launch: ``python bench.py --gpus N --steps K --warmup W``; for N > 1 under
``python -m torch.distributed.run --nproc-per-node N``.  The path shards by subdomain: each
rank owns n lattice layers of one global box that grows with N (weak scaling) plus one halo
layer per cut; assembly needs no collective, the BiCGStab solve (the library's fused loop,
pfv_solve_sharded) exchanges halo entries of the SpMV input point-to-point and fuses every pair of
dot products into one all-reduce - this process only serves those two hooks.

Prints ONE JSON line on rank 0 (contract in the task statement).  A plain run sets up, warms up, times the
``--steps`` steps, optionally writes their outputs (``--dump-outputs DIR``) and prints the headline
(``metric``, ``value``, ``unit``, ``higher_is_better``, ``dtype``, ``ms_per_step``, the configuration of the timed
step).  Everything else is measured only with ``--full``: ``roofline`` for the dominant kernel (CSR SpMV of the
solve; live HIP-event timing through pfv_time_kernel), the cold step, the assembly figures, the field check,
``cpu_baseline`` = PorePy's own CPU path (the reference, byte-compiled by ``oracle/make_ref.py`` into
``oracle/_ref/``) timed on the host cores at 196 608 cells of the same workload family (the oracle port only where
no reference is importable), the whole-grid parity datum and the secondary configurations.

``--dump-outputs DIR`` writes what the last timed step handed its caller, cell by cell in the order of the global
cell ids (the same arrays at any number of ranks): ``pressure.npy`` (the solution), ``rhs.npy`` (the assembled
right-hand side) and ``system_matrix_times_probe.npy`` (the assembled matrix applied to a fixed pseudo-random
vector), float64.  Above 64 MB in all a fixed, seeded sample of the cells is written, their ids in ``cell_ids.npy``.
The inputs of every warmup and timed step are the same from run to run.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8.0 TB/s spec (6.29 TB/s measured copy)


def make_problem(n_side: int, seed: int = 1):
    import porepy_amd as pa

    g = pa.StructuredTetrahedralGrid([n_side] * 3, [1.0, 1.0, 1.0])
    g.compute_geometry()
    g = pa.perturb_interior_nodes(g, 0.2 / n_side, seed=seed)
    nc = g.num_cells
    rng = np.random.default_rng(2)
    scale = np.exp(0.5 * rng.standard_normal(nc))  # mild cell-wise heterogeneity
    K = pa.SecondOrderTensor(kxx=1.0 * scale, kyy=10.0 * scale, kzz=0.1 * scale, kxy=0.5 * scale,
                             kxz=0.05 * scale, kyz=0.2 * scale)
    bf = g.get_all_boundary_faces()
    xf = g.face_centers[0, bf]
    dirf = bf[(xf < 1e-9) | (xf > 1 - 1e-9)]
    bc = pa.BoundaryCondition(g, dirf, ["dir"] * dirf.size)
    bv = np.zeros(g.num_faces)
    bv[dirf] = g.face_centers[0, dirf]
    return g, K, bc, bv, g.cell_volumes.copy()


def bench_config_c2(pa, device_index: int, rtol: float, precond: str, steps: int = 3):
    """BASELINE.json configs[1]: 3-D simplex box, 196 608 tetrahedra ([32]^3 lattice), isotropic K = 1,
    Dirichlet p = x all round -- a secondary line next to the headline workload (configs[2])."""
    g = pa.StructuredTetrahedralGrid([32, 32, 32], [1.0, 1.0, 1.0])
    g.compute_geometry()
    K = pa.SecondOrderTensor(np.ones(g.num_cells))
    bf = g.get_all_boundary_faces()
    bc = pa.BoundaryCondition(g, bf, ["dir"] * bf.size)
    bv = np.zeros(g.num_faces)
    bv[bf] = g.face_centers[0, bf]
    ctx = pa.Context(device_index)
    ctx.set_grid(pa.grid_to_raw(g))
    ctx.set_params(K.values, pa.bc_flags(bc), None, 1.0 / 3.0)
    src = np.zeros(g.num_cells)

    def step():
        ctx.discretize(rebuild_topology=True)
        ctx.assemble(bv, None, src)
        return ctx.solve("bicgstab", rtol=rtol, maxit=20000, raise_on_fail=False, precond=precond)

    x, info = step()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        x, info = step()
    ctx.sync()
    dt = (time.perf_counter() - t0) / steps
    err = float(np.max(np.abs(x - g.cell_centers[0])))  # MPFA reproduces the linear field exactly
    st = ctx.stats()
    return {"workload": "BASELINE configs[1]: 196608 tetrahedra, isotropic K, Dirichlet p = x",
            "value": g.num_cells / dt, "unit": "cells/s", "ms_per_step": 1e3 * dt, "steps": steps,
            "iterations": info["iterations"], "krylov": "bicgstab+" + precond,
            "max_abs_error_vs_exact_linear_field": err,
            "phases_ms": {k: st[k] for k in ("topology_ms", "symbolic_ms", "node_ms", "face_ms", "assemble_ms",
                                             "solve_ms")}}


def bench_config_c4(pa, device_index: int, rtol: float, precond: str, steps: int = 2):
    """BASELINE.json configs[3] on one GPU: MPSA linear elasticity, 511 104 tetrahedra ([44]^3 lattice,
    1.53 M dofs), mu = lambda = 1, rollers on the low faces, unit traction on top; the
    exact solution is the uniaxial field u = (nu x / E, nu y / E, -z / E)."""
    n = 44
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
    bvf = bv.ravel("F")
    ctx = pa.Context(device_index)
    ctx.set_grid(pa.grid_to_raw(g))
    ctx.mpsa_set_params(C.values, g.cell_volumes, bc.is_dir, bc.is_neu, 1.0 / 3.0)

    def step():
        ctx.mpsa_discretize(rebuild_topology=True)
        ctx.mpsa_assemble(bvf, None)
        return ctx.solve("bicgstab", rtol=rtol, maxit=50000, n=3 * nc, raise_on_fail=False, precond=precond)

    for _ in range(2):  # untimed: the handle's block cache has settled after the second step (a miss is a 25 ms hipMalloc)
        u, info = step()
    ctx.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        u, info = step()
    ctx.sync()
    dt = (time.perf_counter() - t0) / steps
    st = ctx.stats()
    cc = g.cell_centers
    E, nu = 2.5, 0.25
    err = float(np.max(np.abs(u.reshape(3, -1, order="F") - np.vstack((nu * cc[0] / E, nu * cc[1] / E, -cc[2] / E)))))
    # interaction-region kernel of MPSA (n = nd x 36 = 108 unknowns at an interior node): FP64 roofline on the
    # executed flops, 2 n^3 for the Gauss-Jordan inverse + ~40 % for the products that follow it
    n_int = (n - 1) ** 3
    mpsa_flops = n_int * 2.0 * 108 ** 3 * 1.4
    node_roofline = {"bound": "mfma", "compute_unit": "FP64 vector FMA (same peak as FP64 MFMA on this part)", "kernel": "mpsa node kernel (512 threads per interaction region; block-cyclic register "
                     "Gauss-Jordan on 256 of them, 8x8 entries per thread, n = 108)", "ms_per_launch": st["node_ms"], "flops_per_launch_estimate": mpsa_flops,
                     "achieved": mpsa_flops / (st["node_ms"] * 1e-3) / 1e12, "peak": 78.6, "unit": "TFLOP/s",
                     "frac": mpsa_flops / (st["node_ms"] * 1e-3) / 78.6e12}
    return {"workload": "BASELINE configs[3] on 1 GPU: MPSA elasticity, 511104 tetrahedra, 3 dof/cell, rollers + top traction",
            "roofline_node_kernel": node_roofline,
            "value": nc / dt, "unit": "cells/s", "ms_per_step": 1e3 * dt, "steps": steps, "dofs": 3 * nc,
            "iterations": info["iterations"], "krylov": "bicgstab+" + precond,
            "node_redo": int(st.get("node_redo", 0)),
            "max_abs_error_vs_exact_uniaxial_field": err,
            "phases_ms": {k: st[k] for k in ("topology_ms", "symbolic_ms", "node_ms", "face_ms", "assemble_ms",
                                             "solve_ms")}}


def _hash_normal(gid: np.ndarray, salt: int) -> np.ndarray:
    """Deterministic N(0,1) per global id (splitmix64 hash + Box-Muller): the same field on every
    rank without materialising a global array."""
    def mix(z):
        z = (z + np.uint64(0x9E3779B97F4A7C15)) & np.uint64(0xFFFFFFFFFFFFFFFF)
        z = ((z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)) & np.uint64(0xFFFFFFFFFFFFFFFF)
        z = ((z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)) & np.uint64(0xFFFFFFFFFFFFFFFF)
        return z ^ (z >> np.uint64(31))
    with np.errstate(over="ignore"):
        g = gid.astype(np.uint64)
        a = mix(g * np.uint64(2) + np.uint64(salt))
        b = mix(g * np.uint64(2) + np.uint64(salt + 1))
    u1 = ((a >> np.uint64(11)).astype(np.float64) + 0.5) / float(1 << 53)
    u2 = ((b >> np.uint64(11)).astype(np.float64) + 0.5) / float(1 << 53)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def permeability_factors(gid: np.ndarray, n_fields: int) -> list:
    """Log-normal factors 1 .. n_fields - 1 of the per-step permeability fields, exp(0.5 N(0,1)) per global cell id,
    drawn by a few host threads (numpy's ufuncs release the GIL): the same arrays as drawn one after the other."""
    from concurrent.futures import ThreadPoolExecutor

    with ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(lambda i: np.exp(0.5 * _hash_normal(gid, 1000 + 2 * i)), range(1, n_fields)))


def block_grid(world: int):
    """(px, py, pz) with px * py * pz = world, as cubic as possible, the largest factor along z (the axis the cells are
    numbered slowest in): 2 -> (1, 1, 2), 4 -> (1, 2, 2), 8 -> (2, 2, 2), 6 -> (1, 2, 3)."""
    best = None
    for px in range(1, world + 1):
        if world % px:
            continue
        for py in range(px, world // px + 1):
            if (world // px) % py:
                continue
            pz = world // (px * py)
            if pz < py:
                continue
            cand = (pz - px, (px, py, pz))
            if best is None or cand < best:
                best = cand
    return best[1]


def make_slab_problem(n_side: int, rank: int, world: int, layers: int | None = None, strong: bool = False,
                      blocks=None):
    """Rank `rank`'s share of the global box [0,1]x[0,1]x[0,layers*world/n] of n x n x (layers*world) lattice
    cells (6 tetrahedra each): its lattice cells plus one halo layer on each interior side,
    built directly (no global grid), owned cells numbered first.  Geometry perturbation and the
    permeability field are functions of GLOBAL node / cell ids, so all ranks see one global problem.
    Default: z-slabs.  ``blocks = (px, py, pz)`` (strong scaling only; px py pz = world): the one-GPU box cut into
    px x py x pz blocks -- at 8 ranks every block of (2, 2, 2) has halo layers on 3 of its 6 sides (9 % more cells to
    discretize than it owns) where an interior slab has them on both sides of its 8-9 layers (23 %).
    Returns (LocalProblem, K values (3,3,nloc), bc flags, bc values, source, eta)."""
    import porepy_amd as pa
    from porepy_amd import distributed as D

    n = n_side
    lay = n if layers is None else int(layers)  # lattice layers owned by each rank (weak scaling)
    ktot = n if strong else lay * world
    dims = (n, n, ktot)
    if blocks is None:
        blocks = (1, 1, world)
    blocks = tuple(int(p) for p in blocks)
    if blocks[0] * blocks[1] * blocks[2] != world:
        raise SystemExit("the block grid does not match the number of ranks")
    if blocks[:2] != (1, 1) and not strong:
        raise SystemExit("blocks in x / y are for strong scaling (weak scaling grows the box along z)")
    # bounds of the ranks along every axis: weak = `lay` layers each along z (the box grows with the number of
    # ranks), strong = the lattice cells of the one-GPU box split as evenly as possible
    bounds = []
    for ax in range(3):
        p = blocks[ax]
        if ax == 2 and not strong:
            bounds.append(lay * np.arange(world + 1))
        else:
            bounds.append(np.array([(r * dims[ax]) // p for r in range(p + 1)]))
        if np.any(np.diff(bounds[ax]) < 1):
            raise SystemExit("more ranks than lattice layers")
    bpos = (rank % blocks[0], (rank // blocks[0]) % blocks[1], rank // (blocks[0] * blocks[1]))
    lo = [int(bounds[ax][bpos[ax]]) for ax in range(3)]
    hi = [int(bounds[ax][bpos[ax] + 1]) for ax in range(3)]
    o0 = [max(0, lo[ax] - 1) for ax in range(3)]            # local lattice range incl. the halo layers
    o1 = [min(dims[ax], hi[ax] + 1) for ax in range(3)]
    nl = [o1[ax] - o0[ax] for ax in range(3)]
    g = pa.StructuredTetrahedralGrid(nl, [nl[0] / n, nl[1] / n, nl[2] / n])
    x = g.nodes.copy()
    for ax in range(3):
        x[ax] += o0[ax] / n
    # global node id and perturbation of globally interior nodes
    nid = np.arange(g.num_nodes)
    il = [nid % (nl[0] + 1), (nid // (nl[0] + 1)) % (nl[1] + 1), nid // ((nl[0] + 1) * (nl[1] + 1))]
    ig = [il[ax] + o0[ax] for ax in range(3)]
    ngid = ig[0] + (n + 1) * (ig[1] + (n + 1) * ig[2])
    interior = np.ones(g.num_nodes, dtype=bool)
    for ax in range(3):
        interior &= (ig[ax] > 0) & (ig[ax] < dims[ax])
    amp = 0.2 / n
    for d in range(3):
        z = _hash_normal(ngid, 100 + 7 * d)
        u = 0.5 * (1.0 + np.tanh(z))  # in (0,1), deterministic per global node
        x[d, interior] += (u[interior] - 0.5) * amp
    g.nodes = x
    g.compute_geometry()
    raw = pa.grid_to_raw(g)
    # cells: local index -> (type, i, j, k) -> global id, ownership
    ncube = nl[0] * nl[1] * nl[2]
    lc = np.arange(g.num_cells)
    t, cube = lc // ncube, lc % ncube
    cl = [cube % nl[0], (cube // nl[0]) % nl[1], cube // (nl[0] * nl[1])]
    cg = [cl[ax] + o0[ax] for ax in range(3)]
    cgid = t + 6 * (cg[0] + n * (cg[1] + n * cg[2]))
    owned = np.ones(g.num_cells, dtype=bool)
    for ax in range(3):
        owned &= (cg[ax] >= lo[ax]) & (cg[ax] < hi[ax])
    # local numbering: owned cells first, each group along a Morton curve (locality of the SpMV gathers)
    io, ih = np.flatnonzero(owned), np.flatnonzero(~owned)
    box = (raw["face_centers"].min(axis=1), raw["face_centers"].max(axis=1))  # the library's quantisation box
    io = io[D.morton_order(raw["cell_centers"][:, io], 3, box)]
    ih = ih[D.morton_order(raw["cell_centers"][:, ih], 3, box)]
    order = np.concatenate([io, ih])
    raw = D.permute_cells(raw, order)
    cgid = cgid[order]
    cg = [c[order] for c in cg]
    n_own = int(owned.sum())
    # faces that are one-sided only because of a cut
    fn_idx = raw["fn_indices"]
    sides = np.bincount(raw["cf_indices"], minlength=g.num_faces)
    artificial = np.zeros(g.num_faces, dtype=bool)
    for ax in range(3):
        fl = il[ax][fn_idx].reshape(g.num_faces, 3)
        artificial |= np.all(fl == 0, axis=1) & (o0[ax] > 0)
        artificial |= np.all(fl == nl[ax], axis=1) & (o1[ax] < dims[ax])
    artificial &= sides == 1
    hown = np.zeros(g.num_cells - n_own, dtype=np.int64)
    stride = 1
    for ax in range(3):
        hown += stride * (np.searchsorted(bounds[ax], cg[ax][n_own:], side="right") - 1)
        stride *= blocks[ax]
    lp = D.LocalProblem(raw=raw, n_own=n_own, cell_gid=cgid.astype(np.int64), halo_owner=hown.astype(np.int32),
                        face_gid=None, artificial_boundary=artificial)
    # parameters: full-tensor anisotropic K times a log-normal field; Dirichlet p = x on x-faces
    scale = np.exp(0.5 * _hash_normal(cgid, 7))
    K = pa.SecondOrderTensor(kxx=1.0 * scale, kyy=10.0 * scale, kzz=0.1 * scale, kxy=0.5 * scale,
                             kxz=0.05 * scale, kyz=0.2 * scale)
    fcx = raw["face_centers"][0]
    true_bnd = (sides == 1) & ~artificial
    dirf = true_bnd & ((fcx < 1e-9) | (fcx > 1 - 1e-9))
    flags = np.zeros(g.num_faces, dtype=np.uint8)
    flags[true_bnd] = 2
    flags[dirf] = 1
    flags[artificial] = 2
    bv = np.zeros(g.num_faces)
    bv[dirf] = fcx[dirf]
    src = raw["cell_volumes"].copy()
    return lp, K.values, flags, bv, src, 1.0 / 3.0


CPU_THREADS = 16  # BLAS / OpenMP threads handed to the reference's CPU run (stated as cpu_baseline.cores)


def cpu_baseline_reference(n_side: int, timeout_s: float = 480.0, num_sub: int = 1, solve_cap_s: float = 0.0):
    """PorePy's OWN scipy/numpy CPU path timed on this box's host cores (kind "reference"):
    ``pp.Mpfa("flow").discretize`` (``mpfa_inverter="python"``: numba is absent) + ``assemble_matrix_rhs`` + the
    linear solve, run by ``oracle/ref_cpu_baseline.py`` in a subprocess that imports the reference from the live
    tree (build container) or from ``oracle/_ref/porepy_ref.zip`` (built by ``oracle/make_ref.py``; the GPU box).
    Same workload family as the timed GPU step at n_side^3*6 cells.  None where no reference is importable."""
    import subprocess

    import oracle

    env = oracle.ref_env()
    if env is None:
        return None
    env["OMP_NUM_THREADS"] = env["OPENBLAS_NUM_THREADS"] = str(CPU_THREADS)
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "oracle", "ref_cpu_baseline.py"), str(n_side),
                            str(num_sub), str(solve_cap_s)],
                           env=env, cwd="/tmp", capture_output=True, text=True, timeout=timeout_s)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if not line:
            return {"error": (r.stderr or "no output")[-400:]}
        o = json.loads(line[-1][7:])
    except Exception as e:
        return {"error": repr(e)}
    total = o["discretize_s"] + o["assemble_s"] + o["solve_s"]
    return {
        "value": o["cells"] / total, "unit": "cells/s",
        # threads the run was given (OMP_NUM_THREADS = OPENBLAS_NUM_THREADS); its hot loops -- scipy's csr_matmat and
        # the Python loop over np.linalg.inv blocks -- are serial, see threads_busy_on_average
        "cores": CPU_THREADS, "threads_busy_on_average": o.get("effective_threads", 1.0), "kind": "reference",
        "num_subproblems": o.get("num_subproblems", 1),
        "sample": f"PorePy itself (imported from {'the byte-compiled archive oracle/_ref' if o['porepy_from'].find('.zip') >= 0 else 'the reference tree'}): "
                  f"{o['cells']} tetrahedra (n_side={n_side}{', BASELINE configs[1] size' if n_side == 32 else ''}) of the timed workload family "
                  f"(perturbed nodes, anisotropic heterogeneous K): pp.Mpfa.discretize {o['discretize_s']:.1f} s "
                  f"(mpfa_inverter='python', numba absent{'' if o.get('num_subproblems', 1) <= 1 else ', partition_arguments num_subproblems=' + str(o['num_subproblems'])}) + assemble_matrix_rhs {o['assemble_s']:.2f} s + solve "
                  f"{o['solve_s']:.1f} s [{o['solver']}; {o['iterations']} iterations, true residual {o['rel_residual']:.1e}]; "
                  f"peak RSS {o['peak_rss_gb']:.1f} GB; host has {o['host_cores']} cores, process CPU time / wall time = "
                  f"{o.get('effective_threads', 1.0):.2f} threads busy (scipy csr_matmat and the Python loop of "
                  "np.linalg.inv are serial; BLAS threads only help the Krylov vectors)",
        "seconds": {"discretize": o["discretize_s"], "assemble": o["assemble_s"], "solve": o["solve_s"]},
        "cells": o["cells"], "check_norm": o["p_norm"], "flux_nnz": o["flux_nnz"],
    }


def cpu_baseline_port(n_side: int):
    """Fallback where the reference is not importable (kind "port"): the oracle (numpy node loop restating the
    reference's algorithm) + scipy direct solve on a bounded sample, 1 thread."""
    import scipy.sparse.linalg as spla

    import porepy_amd as pa
    from oracle import mpfa_oracle as mo

    g, K, bc, bv, src = make_problem(n_side)
    raw = pa.grid_to_raw(g)
    t0 = time.perf_counter()
    mats = mo.discretize(raw, K.values, pa.bc_to_raw(bc))
    A, b = mo.assemble_matrix_rhs(raw, mats, bv)
    t1 = time.perf_counter()
    x = spla.spsolve(A.tocsc(), b + src)
    t2 = time.perf_counter()
    return {
        "value": g.num_cells / (t2 - t0),
        "unit": "cells/s",
        "cores": 1,
        "kind": "port",
        "sample": f"{g.num_cells} tetrahedra (n_side={n_side}) of the same perturbed anisotropic box: "
                  f"oracle discretize+assemble {t1 - t0:.1f} s, scipy spsolve {t2 - t1:.1f} s; "
                  f"host has {os.cpu_count()} cores, path is single-threaded",
        "check_norm": float(np.linalg.norm(x)),
    }


def cpu_baseline(ref_n_side: int, port_n_side: int):
    ref = cpu_baseline_reference(ref_n_side)
    if ref is not None and "error" not in ref:
        return ref
    port = cpu_baseline_port(port_n_side)
    port["reference_unavailable"] = "no reference importable (no /root/reference, no oracle/_ref archive)" if ref is None else ref["error"]
    return port


REFERENCE_HEADLINE_RUN = os.path.join(ROOT, "profiles", "r05_cpu_baseline_headline_grid_cached.json")


def reference_source_digest():
    """sha256 over the reference's source files of the hot path, as recorded by ``oracle/make_ref.py`` inside the
    archive it builds (member ``SOURCE_DIGEST``; the live tree is hashed directly in the build container)."""
    try:
        from oracle import make_ref

        return make_ref.source_digest()
    except Exception:
        return None


def cached_cpu_headline():
    """The reference's CPU path on the HEADLINE grid itself (1 971 054 tetrahedra, ``partition_arguments`` with 12
    sub-problems): 6 minutes of host time, so the default run carries the RECORD of such a run (``--cpu-headline 12``
    measures it live) -- valid for the reference sources whose digest it names."""
    try:
        with open(REFERENCE_HEADLINE_RUN) as fh:
            rec = json.load(fh)
    except Exception:
        return None
    out = dict(rec["cpu_baseline_headline_grid"])
    dig = reference_source_digest()
    out["cached"] = True
    out["record"] = os.path.relpath(REFERENCE_HEADLINE_RUN, ROOT)
    out["measured"] = rec.get("command")
    out["reference_source_digest_of_the_record"] = rec.get("reference_source_digest")
    out["reference_source_digest_here"] = dig
    out["valid_for_this_reference"] = (dig == rec.get("reference_source_digest")) if dig else None
    return out


C5_RECORD = os.path.join(ROOT, "profiles", "r05_c5_32cube_52fractures.json")


def config_c5(live: bool = False):
    """BASELINE configs[4] stand-in at 32^3 (36 657 cells, 98 229 unknowns, 52 fractures, 190 subdomains, 301 interfaces):
    the reference's thermo-hydro model with pp.Mpfa rebound to the library and every Newton system solved on the
    device, beside the untouched reference (tools/c5_bench.py).  The live run takes ~5 minutes of host time (the
    reference's direct solves): ``--c5``; by default the record of such a run on an MI355X box is carried."""
    if live:
        import subprocess

        env = dict(os.environ, C5_N_SIDE="32", C5_MAX_EXTENT="14", PFV_DROPIN_LIBRARY="product")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "c5_bench.py"), "--reference"], env=env,
                           capture_output=True, text=True, timeout=3600)
        line = [l for l in r.stdout.splitlines() if l.startswith("RESULT ")]
        if not line:
            return {"error": (r.stderr or "no output")[-600:]}
        d = json.loads(line[-1][7:])
        live_rec = {"cached": False, "result": d}
        if "error" in d.get("device", {}) or "reference" not in d or "error" in d["reference"]:
            return live_rec
        dev, ref = d["device"], d["reference"]
        live_rec["per_newton_step_s"] = {
            "device": {"assemble_host_ad": dev["seconds"]["assemble"] / dev["calls"]["n_assemble"],
                       "linear_solve_device": dev["seconds"]["solve"] / dev["calls"]["n_solve"]},
            "reference": {"assemble_host_ad": ref["seconds"]["assemble"] / ref["calls"]["n_assemble"],
                          "linear_solve_scipy_direct": ref["seconds"]["solve"] / ref["calls"]["n_solve"]}}
        live_rec["discretize_s"] = {"device_all_190_subdomains": dev["seconds"]["discretize"],
                                    "reference": ref["seconds"]["discretize"]}
        return live_rec
    try:
        with open(C5_RECORD) as fh:
            rec = json.load(fh)
    except Exception:
        return None
    dev, ref = rec["result"]["device"], rec["result"]["reference"]
    return {"cached": True, "record": os.path.relpath(C5_RECORD, ROOT), "measured": rec["command"], "workload": rec["workload"],
            "cells": dev["cells"], "dofs": dev["dofs"], "subdomains": dev["subdomains"], "interfaces": dev["interfaces"],
            "per_newton_step_s": rec["per_newton_step_s"], "discretize_s": rec["discretize_s"],
            "newton_systems": dev["calls"]["n_solve"], "gmres_iterations": dev["gmres_iterations"],
            "worst_true_residual": dev["worst_true_residual"],
            "x_rel_diff_device_vs_reference": rec["result"]["x_rel_diff_device_vs_reference"],
            "reference_source_digest_here": reference_source_digest()}


HEADLINE_PATTERN = os.path.join(ROOT, "tests", "golden", "headline_flux_pattern_69.npz")


N_BLOCKS = 1024


def value_digest(M, n_blocks: int = N_BLOCKS, rows_mask=None):
    """Per block of consecutive rows (n_blocks blocks) of a CSR matrix: sum |a|, sum a^2, and sum a * w(column) with
    w(c) = 0.5 + frac(c * golden ratio) -- fixed weights in [0.5, 1.5) that do not annihilate rows summing to zero.
    The same function makes the reference's fixtures (oracle/gen_golden_headline_pattern.py, gen_golden_mpsa_whole_grid.py,
    gen_golden_biot_whole_grid.py) and digests the device's matrices.  rows_mask: rows that count.  Row chunks of
    2^18 (a 670 M-entry matrix passes with a few hundred MB of work space)."""
    import scipy.sparse as sps

    M = sps.csr_matrix(M)
    n = M.shape[0]
    rows_per = -(-n // n_blocks)
    out = np.zeros((3, n_blocks))
    indptr = np.asarray(M.indptr, dtype=np.int64)
    mask = None if rows_mask is None else np.asarray(rows_mask, bool)
    step = 1 << 18
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        e0, e1 = int(indptr[r0]), int(indptr[r1])
        if e1 == e0:
            continue
        row_of = np.repeat(np.arange(r0, r1, dtype=np.int64), np.diff(indptr[r0:r1 + 1]))
        a = np.asarray(M.data[e0:e1], dtype=float)
        if mask is not None:  # (rows left out: e.g. the Neumann boundary rows of flux, whose true entries are all zero)
            a = np.where(mask[row_of], a, 0.0)
        w = 0.5 + np.mod(M.indices[e0:e1].astype(np.float64) * 0.6180339887498949, 1.0)
        blk = row_of // rows_per
        out[0] += np.bincount(blk, weights=np.abs(a), minlength=n_blocks)
        out[1] += np.bincount(blk, weights=a * a, minlength=n_blocks)
        out[2] += np.bincount(blk, weights=a * w, minlength=n_blocks)
    return out


FINE_ROWS = 256  # rows per block of the fine digest (the 1 024 blocks of value_digest hold 3 878 rows on the headline grid)


def fine_digest(M, rows_mask=None, rows_per: int = FINE_ROWS):
    """Per block of ``rows_per`` consecutive rows: sum |a| and max |a| (a block sum over 3 878 rows x 56
    entries within 1e-13 still lets one entry be off by 2e-8 of a mean entry; 256-row blocks are 15 x tighter, and the
    maximum pins the largest entry of every block on its own).  Same function for the reference's fixture
    (oracle/gen_golden_headline_fine.py) and for the device's matrices."""
    import scipy.sparse as sps

    M = sps.csr_matrix(M)
    n = M.shape[0]
    nb = -(-n // rows_per)
    out = np.zeros((2, nb))
    indptr = np.asarray(M.indptr, dtype=np.int64)
    mask = None if rows_mask is None else np.asarray(rows_mask, bool)
    step = 1 << 18
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        e0, e1 = int(indptr[r0]), int(indptr[r1])
        if e1 == e0:
            continue
        row_of = np.repeat(np.arange(r0, r1, dtype=np.int64), np.diff(indptr[r0:r1 + 1]))
        a = np.abs(np.asarray(M.data[e0:e1], dtype=float))
        if mask is not None:
            a = np.where(mask[row_of], a, 0.0)
        blk = row_of // rows_per
        out[0] += np.bincount(blk, weights=a, minlength=nb)
        np.maximum.at(out[1], blk, a)
    return out


def vector_digest(x, n_blocks: int = N_BLOCKS):
    """Per block of consecutive entries: sum x, sum x^2."""
    x = np.asarray(x, dtype=float)
    rows_per = -(-x.size // n_blocks)
    blk = np.arange(x.size, dtype=np.int64) // rows_per
    return np.stack([np.bincount(blk, weights=x, minlength=n_blocks), np.bincount(blk, weights=x * x, minlength=n_blocks)])


def whole_grid_check(pa, device_index: int, rtol: float, precond: str, want_pattern: bool = False, n_side: int = 69,
                     library=None, fixture: str | None = None, fine_fixture: str | None = None):
    """Whole-grid parity datum at the headline size.  The REFERENCE was run on all 1 971 054
    tetrahedra of make_problem(69) (``oracle/gen_golden_headline_pattern.py``: pp.Mpfa with 12 sub-problems, 20 minutes
    of host time; the same topology and geometry arrays the device gets) and left, in
    tests/golden/headline_flux_pattern_69.npz, the number of entries it STORES in every one of the 3 970 674 rows of
    ``flux`` and a digest of their (row, column) pairs.  Here: the device's flux pattern on the same grid must have
    exactly those row lengths in every row that is not a Neumann boundary row (where the true entries are all zero
    and what either side stores is cancellation noise: there the reference's stored entries are a subset)."""
    z = np.load(fixture or (HEADLINE_PATTERN if n_side == 69 else HEADLINE_PATTERN.replace("_69.npz", f"_{n_side}.npz")))
    tot = json.loads(str(z["totals"]))
    t0 = time.perf_counter()
    g, K, bc, bv, src = make_problem(n_side)
    nf = g.num_faces
    ref_len = z["row_len"].astype(np.int64)
    neu = np.unpackbits(z["neumann_row"])[:nf].astype(bool)
    ctx = pa.Context(device_index) if library is None else pa.Context(device_index, library)
    try:
        ctx.set_grid(pa.grid_to_raw(g))
        ctx.set_params(K.values, pa.bc_flags(bc), None, 1.0 / 3.0)
        ctx.discretize(rebuild_topology=True)
        ctx.assemble(bv, None, src)
        x, info = ctx.solve("bicgstab", rtol=rtol, maxit=20000, raise_on_fail=False, precond=precond)
        F = ctx.matrix(pa._lib.MAT_FLUX)
        BF = ctx.matrix(pa._lib.MAT_BOUND_FLUX) if "flux_value_digest" in z.files else None
        more = {}
        if "vector_source_value_digest" in z.files:  # (all six matrices: digested one at a time, 8 GB each for the largest)
            for name, which, msk in (("bound_pressure_cell", pa._lib.MAT_BOUND_PRESSURE_CELL, None),
                                     ("bound_pressure_face", pa._lib.MAT_BOUND_PRESSURE_FACE, None),
                                     ("vector_source", pa._lib.MAT_VECTOR_SOURCE, ~neu),
                                     ("bound_pressure_vector_source", pa._lib.MAT_BOUND_PRESSURE_VECTOR_SOURCE, None)):
                Mx = ctx.matrix(which)
                more[name] = value_digest(Mx, z[name + "_value_digest"].shape[1], rows_mask=msk)
                del Mx
        # fine datum of a second run of the reference on the same grid (round 6: oracle/gen_golden_headline_fine.py): per
        # block of 256 rows sum |a| and max |a| of all six matrices
        fine = {}
        fpath = fine_fixture or HEADLINE_PATTERN.replace("headline_flux_pattern_", "headline_fine_digest_").replace("_69.npz", f"_{n_side}.npz")
        if os.path.exists(fpath) and (fixture is None or fine_fixture is not None):
            zf = np.load(fpath)
            for name, which, msk in (("flux", pa._lib.MAT_FLUX, ~neu), ("bound_flux", pa._lib.MAT_BOUND_FLUX, None),
                                     ("bound_pressure_cell", pa._lib.MAT_BOUND_PRESSURE_CELL, None),
                                     ("bound_pressure_face", pa._lib.MAT_BOUND_PRESSURE_FACE, None),
                                     ("vector_source", pa._lib.MAT_VECTOR_SOURCE, ~neu),
                                     ("bound_pressure_vector_source", pa._lib.MAT_BOUND_PRESSURE_VECTOR_SOURCE, None)):
                if name + "_fine" not in zf.files:
                    continue
                Mx = F if name == "flux" else ctx.matrix(which)
                dev, ref = fine_digest(Mx, rows_mask=msk), zf[name + "_fine"]
                if name != "flux":
                    del Mx
                gscale = float(np.max(ref[1]))  # (largest entry of the matrix: blocks of boundary rows hold tiny sums)
                sc0 = np.maximum(ref[0], 1e-6 * gscale)
                fine[name] = {"blocks": int(ref.shape[1]),
                              "sum_abs_worst_rel_diff": float(np.max(np.abs(dev[0] - ref[0]) / sc0)),
                              "max_abs_worst_rel_diff": float(np.max(np.abs(dev[1] - ref[1]) / np.maximum(ref[1], 1e-6 * gscale)))}
        nnz_sys = int(ctx.matrix_info(pa._lib.MAT_SYSTEM)[2])
    finally:
        ctx.close()
    dev_len = np.diff(F.indptr).astype(np.int64)
    out = {"grid": "make_problem(69): 1 971 054 tetrahedra, the grid the reference was run on as a whole "
                   "(oracle/gen_golden_headline_pattern.py; same lattice and stencil as the timed grid, nodes and K "
                   "drawn from numpy's generator)",
           "cells": int(g.num_cells), "faces": int(nf),
           "flux_nnz_device": int(F.nnz), "flux_nnz_reference": int(tot["flux_nnz"]),
           "rows_outside_neumann_boundary": int((~neu).sum()),
           "flux_nnz_outside_neumann_rows_device": int(dev_len[~neu].sum()),
           "flux_nnz_outside_neumann_rows_reference": int(tot["flux_nnz_outside_neumann_rows"]),
           "rows_with_a_different_length_outside_neumann_rows": int((dev_len[~neu] != ref_len[~neu]).sum()),
           "neumann_rows_where_the_reference_stores_more": int((ref_len[neu] > dev_len[neu]).sum()),
           "system_nnz_device": nnz_sys, "p_norm_device": float(np.linalg.norm(x)),
           "device_iterations": int(info["iterations"]), "device_rel_residual": float(info["rel_residual"]),
           "reference_discretize_s_on_the_build_host": tot["discretize_s"],
           "seconds_incl_host_grid": time.perf_counter() - t0}
    out["pattern_row_lengths_equal"] = (out["rows_with_a_different_length_outside_neumann_rows"] == 0 and
                                        out["neumann_rows_where_the_reference_stores_more"] == 0)
    if "flux_value_digest" in z.files:
        # VALUE datum of the same reference run (round 5, late): per block of consecutive rows (1024 blocks) sum |a|,
        # sum a^2 and a column-weighted sum of flux and bound_flux, and the pressure field of the reference's own
        # assemble_matrix_rhs + scipy BiCGStab (rtol 1e-13) -- relative differences, block by block
        def worst(dev, ref):
            scale = np.maximum(np.abs(ref[0]), 1e-300)  # (sum |a| of the block: the scale of all three rows)
            return [float(np.max(np.abs(dev[0] - ref[0]) / scale)),
                    float(np.max(np.abs(dev[1] - ref[1]) / np.maximum(np.abs(ref[1]), 1e-300))),
                    float(np.max(np.abs(dev[2] - ref[2]) / scale))]

        out["values_vs_reference"] = {
            "blocks": int(z["flux_value_digest"].shape[1]),
            "flux_worst_rel_diff_abs_sq_weighted": worst(value_digest(F, rows_mask=~neu), z["flux_value_digest"]),
            "bound_flux_worst_rel_diff_abs_sq_weighted": worst(value_digest(BF), z["bound_flux_value_digest"]),
            **{k + "_worst_rel_diff_abs_sq_weighted": worst(v, z[k + "_value_digest"]) for k, v in more.items()},
            "pressure_norm_reference": float(z["pressure_norm"][0]),
            "pressure_norm_rel_diff": float(abs(np.linalg.norm(x) - z["pressure_norm"][0]) / z["pressure_norm"][0]),
            "reference_solve": json.loads(str(z["solve"])),
        }
        pd, pr = vector_digest(x), z["pressure_digest"]
        out["values_vs_reference"]["pressure_block_sums_worst_rel_diff"] = float(
            np.max(np.abs(pd[0] - pr[0]) / np.maximum(np.sqrt(pr[1] * np.maximum(1, -(-x.size // pr.shape[1]))), 1e-300)))
        out["values_vs_reference"]["pressure_block_squares_worst_rel_diff"] = float(
            np.max(np.abs(pd[1] - pr[1]) / np.maximum(pr[1], 1e-300)))
    if fine:
        out["fine_values_vs_reference"] = {"rows_per_block": FINE_ROWS, **fine}
    if want_pattern:
        out["_pattern"] = (F.indptr, F.indices, ~neu, int(z["digest_rows"][0]))
    return out


def source_hash() -> str:
    """Digest of the kernel sources: PMC files under profiles/ carry it, so counters are only quoted for the
    build they were collected with."""
    import hashlib

    h = hashlib.sha256()
    d = os.path.join(ROOT, "porepy_amd", "csrc")
    for f in sorted(os.listdir(d)):
        if f.endswith((".hip", ".inc", ".h")):
            h.update(open(os.path.join(d, f), "rb").read())
    return h.hexdigest()[:16]


def load_pmc(n_side: int, world: int) -> dict:
    """HBM traffic per launch from the PMC passes of tools/gpu_pmc.sh (FETCH_SIZE and WRITE_SIZE in separate
    runs), if profiles/ holds a file collected with exactly this build on this workload; else {}."""
    for name in ("r06_pmc_traffic.json", "r05_pmc_traffic.json"):  # (the newest file collected with THIS build wins)
        try:
            with open(os.path.join(ROOT, "profiles", name)) as fh:
                pj = json.load(fh)
            if pj.get("n_side") == n_side and world == 1 and pj.get("source_hash") == source_hash():
                return pj["kernels"]
        except Exception:
            pass
    return {}


def bench_operator_api(pa, lp, Kvals, flags, bv, src, eta, device_index: int):
    """The drop-in surface itself on the headline grid: `Mpfa(kw).discretize(g, data)` +
    `assemble_matrix_rhs(g, data)` with host arrays in and scipy matrices out (fv_elliptic.py:67-112), grid
    already uploaded (the first call uploads it).  `eager`: all six matrices copied to the host, as the
    reference leaves them in `data`; `lazy`: `Mpfa(kw, lazy=True)`, proxies that fetch on first use -- only A
    and b cross PCIe."""
    import gc

    g = pa.grid_from_raw(lp.raw)
    K = type("K", (), {"values": Kvals})()
    bc = type("BC", (), {"is_dir": (flags & 1) != 0, "is_neu": (flags & 2) != 0, "is_rob": np.zeros(flags.size, bool),
                         "is_internal": np.zeros(flags.size, bool), "robin_weight": np.ones(flags.size)})()
    out = {}
    d = pa.Mpfa("flow", device_index, lazy=True)
    data = pa.initialize_data({}, "flow", {"second_order_tensor": K, "bc": bc, "bc_values": bv,
                                            "hip_rebuild_topology": True, "mpfa_eta": eta})
    d.discretize(g, data)  # uploads the grid (untimed: the headline step also starts with the grid in HBM)
    A, b = d.assemble_matrix_rhs(g, data)
    pool = pa._lib.pinned_pool(d.context(g).lib)
    for mode, reps in (("lazy", 2), ("eager", 1)):
        d.lazy = mode == "lazy"
        first_ms = None
        if mode == "eager":
            # first eager call of the process: the page-locked blocks of the six matrices are allocated here (the
            # blocks of A and b already sit in the pool); every later call -- a time-stepping loop -- finds them
            md = A = b = None
            gc.collect()
            tf = time.perf_counter()
            d.discretize(g, data)
            A, b = d.assemble_matrix_rhs(g, data)
            first_ms = 1e3 * (time.perf_counter() - tf)
            md = A = b = None
            data[pa.DISCRETIZATION_MATRICES]["flow"] = {}
            gc.collect()
        t0 = time.perf_counter()
        for _ in range(reps):
            d.discretize(g, data)
            A, b = d.assemble_matrix_rhs(g, data)
        dt = (time.perf_counter() - t0) / reps
        md = data[pa.DISCRETIZATION_MATRICES]["flow"]
        out[mode] = {"ms": 1e3 * dt, "value": g.num_cells / dt, "unit": "cells/s",
                     "host_bytes_out": float(A.data.nbytes + A.indices.nbytes + A.indptr.nbytes + b.nbytes +
                                             (0 if mode == "lazy" else sum(m.data.nbytes + m.indices.nbytes + m.indptr.nbytes
                                                                           for m in md.values())))}
        if first_ms is not None:
            out[mode]["first_call_ms"] = first_ms
    out["pinned_pool"] = {"blocks_page_locked": pool.allocated, "requests_served_from_pool": pool.reused,
                          "note": "result arrays are page-locked blocks recycled through porepy_amd._lib.PinnedPool "
                                  "(PFV_PINNED_POOL=0: pageable numpy arrays, 23 GB/s and first-touch page faults)"}
    del d, data, A, b, md
    gc.collect()
    out["workload"] = "Mpfa('flow').discretize(g, data) + assemble_matrix_rhs(g, data) on the headline grid, host arrays in, scipy csr out"
    return out


DUMP_BYTES_MAX = 64 << 20  # --dump-outputs: at most 64 MB in all
DUMP_PROBE_SALT = 4242     # the probe vector the assembled matrix is applied to: _hash_normal(global cell id, salt)
DUMP_SAMPLE_SEED = 20250611


def dump_outputs(out_dir: str, pa, ctx, x, lp, dist, rank: int):
    """--dump-outputs: what the last timed step handed its caller -- the solution, the assembled right-hand side and the
    assembled matrix applied to a fixed probe vector (a function of the global cell id) -- for the cells each rank owns,
    gathered on rank 0 and written in the order of the global cell ids as float64.  Above DUMP_BYTES_MAX in all: a
    fixed, seeded sample of the cells, their global ids in cell_ids.npy."""
    n = lp.n_own
    gid = np.asarray(lp.cell_gid, dtype=np.int64)
    xh = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
    probe = _hash_normal(gid, DUMP_PROBE_SALT)
    mine = (gid[:n], {"pressure": np.array(xh[:n], dtype=np.float64),
                      "rhs": np.array(ctx.rhs()[:n], dtype=np.float64),
                      "system_matrix_times_probe": np.array(ctx.spmv(pa._lib.MAT_SYSTEM, probe)[:n], dtype=np.float64)})
    parts = [mine]
    if dist is not None:
        parts = [None] * dist.get_world_size()
        dist.all_gather_object(parts, mine)
    if rank != 0:
        return
    ids = np.concatenate([p[0] for p in parts])
    order = np.argsort(ids, kind="stable")
    out = {k: np.concatenate([p[1][k] for p in parts])[order] for k in mine[1]}
    if 8 * len(out) * ids.size > DUMP_BYTES_MAX:
        m = DUMP_BYTES_MAX // (8 * (len(out) + 1))
        pick = np.sort(np.random.default_rng(DUMP_SAMPLE_SEED).choice(ids.size, m, replace=False))
        out = {k: v[pick] for k, v in out.items()}
        out["cell_ids"] = ids[order][pick].astype(np.float64)
    os.makedirs(out_dir, exist_ok=True)
    for k, v in out.items():
        np.save(os.path.join(out_dir, k + ".npy"), v)


def self_launch_if_needed():
    """``python bench.py --gpus N`` with N > 1 and no launcher around it (WORLD_SIZE unset): start the N ranks of
    this node here -- the same ``python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr
    127.0.0.1`` line the contract names, replacing this process, so rank 0's JSON line is this command's stdout."""
    if "WORLD_SIZE" in os.environ or "RANK" in os.environ:
        return
    n = 1
    for i, a in enumerate(sys.argv):
        if a == "--gpus" and i + 1 < len(sys.argv):
            n = int(sys.argv[i + 1])
        elif a.startswith("--gpus="):
            n = int(a.split("=", 1)[1])
    if n <= 1:
        return
    import socket

    with socket.socket() as sk:  # a free rendezvous port
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env["PFV_BENCH_SELF_LAUNCHED"] = "1"
    print("bench.py: launching", " ".join(cmd), file=sys.stderr, flush=True)
    os.execvpe(cmd[0], cmd, env)


def main():
    self_launch_if_needed()
    # stdout carries exactly one line, the JSON record: everything else this process or its libraries print
    # (RCCL writes a version banner to the C-level stdout when a communicator is created) goes to stderr
    sys.stdout.flush()
    record_out = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n-side", type=int, default=69, help="lattice cells per side (6 tets each)")
    ap.add_argument("--rtol", type=float, default=1e-13,
                    help="relative tolerance on the TRUE residual; 1e-13 is what 1e-10 field parity needs (SURVEY 8(d))")
    ap.add_argument("--partition", choices=("auto", "slabs", "blocks"), default="auto",
                    help="N > 1: how the box is cut -- z-slabs, or px x py x pz blocks as cubic as possible (2x2x2 at 8 "
                         "ranks: 9 %% instead of 23 %% halo cells); auto = blocks for strong scaling, slabs for weak")
    ap.add_argument("--precond", choices=("amg", "amg_block", "jacobi"), default="amg",
                    help="preconditioner of the BiCGStab solve: aggregation-AMG cycle (default; N > 1: the coupled "
                         "hierarchy, halo exchange on every level), amg_block (N > 1 only: block Jacobi across ranks, "
                         "the hierarchy of each rank's diagonal block) or Jacobi")
    ap.add_argument("--cpu-n-side", type=int, default=32,
                    help="lattice side of the reference's CPU run (32 = 196 608 cells, BASELINE configs[1] size: ~2 min)")
    ap.add_argument("--cpu-port-n-side", type=int, default=16, help="size of the oracle-port fallback")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-headline", type=int, default=0, metavar="K",
                    help="also time the reference on the HEADLINE grid itself (configs[2] size) with "
                         "partition_arguments={'num_subproblems': K} (SURVEY 8(d)); minutes of host time: off by default, "
                         "the record of such a run is kept under profiles/")
    ap.add_argument("--c5", action="store_true",
                    help="run the configs[4] stand-in (52 fractures, 32^3) live: device-backed model and the reference, "
                         "~5 minutes; by default the bench line carries the record under profiles/")
    ap.add_argument("--fixed-k", action="store_true",
                    help="repeat the step on ONE permeability field (rounds 1-4) instead of a new field per step")
    ap.add_argument("--no-cold", action="store_true", help="skip the secondary figure ms_per_step_cold")
    ap.add_argument("--no-whole-grid-check", action="store_true",
                    help="skip the whole-grid parity datum against the recorded reference run (profiling runs)")
    ap.add_argument("--phases", action="store_true", help="also print per-phase timings to stderr")
    ap.add_argument("--no-extra-configs", action="store_true",
                    help="skip the secondary lines for BASELINE configs[1] and configs[3] (profiling runs)")
    ap.add_argument("--scaling", choices=("weak", "strong"), default="strong",
                    help="strong (default, what the north-star target is quoted on): the one-GPU box of --n-side "
                         "split into N slabs; weak: every GPU owns an n x n x n lattice slab of a box that grows with N")
    ap.add_argument("--force-sharded", action="store_true",
                    help="run the N > 1 code path (torch-driven sharded solver) on one GPU, for validation")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure and check everything beside the headline: cold step, "
                         "rooflines, assembly figures, field check, CPU baselines, whole-grid datum, secondary "
                         "configurations (the --no-* / --cpu-* / --c5 options tune these)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the arrays the last timed step computed as DIR/<name>.npy (float64, at most 64 MB)")
    args = ap.parse_args()

    import torch

    import porepy_amd as pa

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    # validation hook for boxes with fewer GPUs than ranks (never set by the driver): all ranks share
    # GPU 0 and talk over gloo, which exercises everything of the N > 1 path except RCCL itself
    share_gpu = os.environ.get("PFV_BENCH_SHARE_GPU", "0") in ("1", "rccl")
    share_rccl = os.environ.get("PFV_BENCH_SHARE_GPU", "0") == "rccl"  # try RCCL itself with both ranks on GPU 0
    if share_gpu:
        local_rank = 0
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch N > 1 with python -m torch.distributed.run --nproc-per-node N")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback)")
    torch.cuda.set_device(local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist_mod

        dist = dist_mod
        if share_gpu and not share_rccl:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    from porepy_amd import distributed as D

    blocks = None  # z-slabs
    if args.partition == "blocks" or (args.partition == "auto" and args.scaling == "strong"):
        if args.scaling != "strong":
            raise SystemExit("--partition blocks cuts the one-GPU box: it needs --scaling strong")
        blocks = block_grid(world)
    lp, Kvals, flags, bv, src, eta = make_slab_problem(args.n_side, rank, world, strong=args.scaling == "strong",
                                                       blocks=blocks)
    nc = lp.n_own                      # cells this rank owns (halo cells are recomputed, not counted)
    nloc = lp.raw["cell_centers"].shape[1]
    if world == 1 and not args.force_sharded:
        ctx = pa.Context(local_rank)
        ctx.set_grid(lp.raw)
        ctx.set_params(Kvals, flags, None, eta)
        sh = None

        # inputs resident in HBM when the timed region starts, solution left in HBM (torch only owns the buffers)
        dev = torch.device("cuda", local_rank)
        d_bv = torch.from_numpy(np.ascontiguousarray(bv, dtype=np.float64)).to(dev)
        d_src = torch.from_numpy(np.ascontiguousarray(src, dtype=np.float64)).to(dev)
        d_x = torch.zeros(nloc, dtype=torch.float64, device=dev)
        torch.cuda.synchronize()

        # A NEW permeability field in every step: the log-normal factor is re-drawn per step from
        # the global cell ids (same sparsity pattern, every VALUE moves), generated before the timed region and resident
        # in HBM; the step forms K_i = K_aniso x factor_i on the device and hands it over device-to-device
        # (pfv_mpfa_set_permeability).  Whatever the library keeps between steps is therefore kept across MOVING values.
        n_fields = 1 if args.fixed_k else min(64, 6 + args.warmup + args.steps + 1)
        base_scale = np.exp(0.5 * _hash_normal(lp.cell_gid, 7))
        d_aniso = torch.from_numpy(np.ascontiguousarray(Kvals / base_scale[None, None, :])).to(dev)   # (3, 3, nloc)
        fields = [base_scale] + permeability_factors(lp.cell_gid, n_fields)
        d_fac = torch.from_numpy(np.ascontiguousarray(np.stack(fields))).to(dev)                      # (n_fields, nloc)
        d_K = torch.empty_like(d_aniso)
        del fields
        step_no = [0]
        torch.cuda.synchronize()

        def set_field(i):
            torch.mul(d_aniso, d_fac[i % n_fields][None, None, :], out=d_K)
            torch.cuda.current_stream().synchronize()   # (torch's stream -> the handle's stream)
            ctx.set_permeability_device(d_K.data_ptr())

        def step():
            step_no[0] += 1
            set_field(step_no[0])
            ctx.discretize(rebuild_topology=True)
            ctx.assemble_device(d_bv.data_ptr(), 0, d_src.data_ptr())
            info = ctx.solve_device(d_x.data_ptr(), "bicgstab", rtol=args.rtol, maxit=20000, raise_on_fail=False,
                                    precond=args.precond)
            return d_x, info
    else:
        sh = D.ShardedMpfa(lp, device=f"cuda:{local_rank}", local_device_index=local_rank, dist=dist)
        ctx = sh.ctx

        # as in the one-GPU path: vector inputs resident in HBM when the timed region starts, the solution
        # stays there; the Krylov loop is the library's fused one (pfv_solve_sharded), this process only
        # serves its two exchange hooks (halo entries point-to-point, one all-reduce per pair of dots)
        devs = torch.device("cuda", local_rank)
        d_bv = torch.from_numpy(np.ascontiguousarray(bv, dtype=np.float64)).to(devs)
        d_src = torch.from_numpy(np.ascontiguousarray(src, dtype=np.float64)).to(devs)
        torch.cuda.synchronize()
        drv = os.environ.get("PFV_SHARDED_DRIVER", "library")

        # as above: a new log-normal factor per step, a function of the GLOBAL cell ids (one global field on all ranks)
        n_fields = 1 if args.fixed_k else min(32, 6 + args.warmup + args.steps + 1)
        base_scale = np.exp(0.5 * _hash_normal(lp.cell_gid, 7))
        d_aniso = torch.from_numpy(np.ascontiguousarray(Kvals / base_scale[None, None, :])).to(devs)
        fields = [base_scale] + permeability_factors(lp.cell_gid, n_fields)
        d_fac = torch.from_numpy(np.ascontiguousarray(np.stack(fields))).to(devs)
        d_K = torch.empty_like(d_aniso)
        del fields
        step_no = [0]
        # (conditions and eta go up once, with host arrays; every step then replaces the permeability device to device)
        sh.discretize(Kvals, flags, None, eta, skip_vector_source=False, rebuild_topology=True)
        torch.cuda.synchronize()

        def step():
            step_no[0] += 1
            torch.mul(d_aniso, d_fac[step_no[0] % n_fields][None, None, :], out=d_K)
            sh.discretize(d_K, flags, None, eta, skip_vector_source=False, rebuild_topology=True)
            sh.assemble(d_bv, d_src)
            return sh.solve("bicgstab", rtol=args.rtol, maxit=20000, precond=args.precond, driver=drv)

    # Untimed pre-warm, before (and not counted among) the W warmup steps: the first process on a fresh box
    # has been seen running its launch-bound phases at half speed for its first seconds (busy host, cold
    # caches); repeat the step until two consecutive step times agree.  Every rank takes the same
    # decision (the sharded step contains collectives).
    prewarm = 0
    if os.environ.get("PFV_BENCH_PREWARM", "1") != "0":
        last = None
        for _ in range(6):
            barrier()
            tp = time.perf_counter()
            step()
            ctx.sync()
            torch.cuda.synchronize()
            dtp = time.perf_counter() - tp
            prewarm += 1
            stable = 1 if (last is not None and abs(dtp - last) <= 0.05 * last) else 0
            if dist is not None:
                tst = torch.tensor([stable], dtype=torch.int32, device="cuda")
                dist.all_reduce(tst, op=dist.ReduceOp.MIN)
                stable = int(tst.item())
            last = dtp
            if stable:
                break
    step_no[0] = 0  # (the warmup and timed steps draw the same fields in every run, however long the pre-warm took)
    for _ in range(args.warmup):
        x, info = step()
    barrier()
    t0 = time.perf_counter()
    each = []   # (the solve call returns once the host has read its iteration count: a step is synchronous)
    for _ in range(args.steps):
        ts = time.perf_counter()
        x, info = step()
        each.append((1e3 * (time.perf_counter() - ts), int(info["iterations"]) if isinstance(info, dict) and "iterations" in info else -1))
    ctx.sync()
    barrier()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device="cuda")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    st = ctx.stats()
    ms_per_step = 1e3 * elapsed / args.steps
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, pa, ctx, x, lp, dist, rank)
    # ---- the same step with NOTHING kept between steps (aggregate maps, SpMV windows, filter layout, Galerkin sizes
    # all rebuilt): the cold figure beside the headline
    cold = None
    if args.full and not args.no_cold:
        off = {"PFV_AMG_REUSE_REBUILT": "0", "PFV_WIN_REUSE": "0", "PFV_AMG_FILTER_LAYOUT_REUSE": "0", "PFV_AMG_SIZES_REUSE": "0",
               "PFV_SYMB_REUSE": "0"}
        saved = {k: os.environ.get(k) for k in off}
        os.environ.update(off)
        try:
            step()
            barrier()
            tc0 = time.perf_counter()
            ncold = max(2, min(args.steps, 5))
            for _ in range(ncold):
                xc, infoc = step()
            ctx.sync()
            barrier()
            tcold = time.perf_counter() - tc0
            if dist is not None:
                tt = torch.tensor([tcold], dtype=torch.float64, device="cuda")
                dist.all_reduce(tt, op=dist.ReduceOp.MAX)
                tcold = float(tt.item())
            stc = ctx.stats()
            cold = {"ms_per_step_cold": 1e3 * tcold / ncold, "steps": ncold,
                    "iterations": int(infoc["iterations"]) if isinstance(infoc, dict) else None,
                    "amg_setup_ms": stc["amg_setup_ms"], "kept": {"amg_aggregate_maps": int(stc.get("amg_maps_reused", 0)),
                                                                   "spmv_windows": int(stc.get("win_reused", 0)),
                                                                   "csr_patterns": int(stc.get("symbolic_reused", 0)),
                                                                   "amg_filter_layout": int(stc.get("amg_filter_layout", 0))},
                    "switches": off}
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
        step()             # (patterns built under PFV_SYMB_REUSE=0 carry no key: this step rebuilds them WITH one)
        x, info = step()   # (back to the default step: the diagnostics below look at its state)
        ctx.sync()
        st = ctx.stats()
    ncells_total = nc
    if dist is not None:
        tcount = torch.tensor([nc], dtype=torch.int64, device="cuda")
        dist.all_reduce(tcount)
        ncells_total = int(tcount.item())
    value = ncells_total * args.steps / elapsed

    its = int(info["iterations"]) if isinstance(info, dict) and "iterations" in info else 0
    # ---- everything beside the headline (--full): cold step above, rooflines, assembly figures, checks, baselines,
    # secondary configurations
    kernels, roofline, per_step_ms, triad_gbs, read_gbs, assembly = [], None, None, None, None, None
    cpu = c2 = c4 = opapi = field = cpu_headline = whole_grid = per_rank = None
    if args.full:
        # ---- rooflines: every kernel that matters, the one with the most time per step is `roofline` ----
        triad_ms = ctx.time_kernel(4, reps=10)
        triad_gbs = 3.0 * 8.0 * (1 << 27) / (triad_ms * 1e-3) / 1e9  # a = b + s c on 3 x 2^27 doubles
        read_gbs = 8.0 * (1 << 28) / (ctx.time_kernel(5, reps=10) * 1e-3) / 1e9  # read-only stream over 2^28 doubles
        pmc = load_pmc(args.n_side, world)

        def hbm_entry(name, kernel, bytes_per_launch, ms, launches_per_step, note, pmc_key=None, extra=None):
            ach = bytes_per_launch / (ms * 1e-3) / 1e9
            e = {"bound": "hbm", "kernel": kernel, "achieved": ach, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                 "frac": ach / HBM_PEAK_GBS, "frac_of_measured_triad": ach / triad_gbs,
                 "frac_of_measured_read_stream": ach / read_gbs,
                 "traffic": (pmc.get(pmc_key, {}) or {}).get("traffic_bytes_per_launch") if pmc_key else None,
                 "bytes_per_launch": bytes_per_launch, "ms_per_launch": ms, "launches_per_step": launches_per_step,
                 "ms_per_step": ms * launches_per_step, "note": note, "name": name}
            if extra:
                e.update(extra)
            return e

        _, _, nnzA = ctx.matrix_info(pa._lib.MAT_SYSTEM)
        kernels = []
        spmv_ms = ctx.time_kernel(0, reps=50)
        spmv_bytes = 12.0 * nnzA + 4.0 * (nloc + 1) + 8.0 * nloc + 8.0 * nloc  # values+indices, indptr, x, y
        # launches per step: two products per BiCGStab iteration + the product of the true-residual check that ends every
        # solve (linalg.inc: krylov_solve, PFV_TRUE_RESIDUAL) -- the same kernel on the same matrix
        true_residual_products = 0 if (sh is not None or os.environ.get("PFV_TRUE_RESIDUAL", "1") == "0") else 1
        kernels.append(hbm_entry(
            "krylov_f64_product", "k_spmv_win<double> (CSR SpMV with A in f64, x window staged in LDS, fused dots)",
            spmv_bytes, spmv_ms, 2 * its + true_residual_products,
            "achieved = SURVEY 8(d) CSR bytes (12 B per entry) / time; the kernel itself streams ~10 B per entry "
            "(16-bit window-local column indices)", "krylov",
            {"streamed_GBs": (10.0 * nnzA + 4.0 * (nloc + 1) + 8.0 * nloc + 12.0 * nloc * 0.36) / (spmv_ms * 1e-3) / 1e9}))
        if args.precond in ("amg", "amg_block") and os.environ.get("PFV_AMG_FP32", "1") != "0":
            sm_ms = ctx.time_kernel(3, reps=50)
            st_amg = ctx.stats()
            nnzS = int(st_amg.get("amg_level0_nnz", 0)) or nnzA  # the cycle's finest level: the strength-filtered operator
            sm_bytes = 8.0 * nnzS + 4.0 * (nloc + 1) + 4 * 8.0 * nloc  # f32 values + indices, indptr, x, y, b, dinv
            kernels.append(hbm_entry(
                "amg_f32_smoothing_product", "k_spmv_win<float, smooth> (finest-level smoothing product of the AMG cycle: "
                "y = x + w D^-1 (b - A_s x), f32 matrix values, f64 vectors)", sm_bytes, sm_ms, 4 * its,
                f"achieved = CSR bytes with f32 values (8 B per entry) / time; the kernel streams ~6 B per entry.  A_s = the "
                f"strength-filtered copy of A the cycle works on (theta {st_amg.get('amg_filter_theta', 0.0):.3f}: {nnzS} of "
                f"{nnzA} entries; the Krylov product keeps A)", "smooth",
                {"streamed_GBs": (6.0 * nnzS + 4.0 * (nloc + 1) + 4 * 8.0 * nloc + 12.0 * nloc * 0.36) / (sm_ms * 1e-3) / 1e9,
                 "entries": nnzS}))
        nnz = {k: ctx.matrix_info(i)[2] for i, k in enumerate(("flux", "bound_flux", "bpc", "bpf", "vs", "bpvs"))}
        face_ms = ctx.time_kernel(2, reps=3)
        face_bytes = 8.0 * sum(nnz.values())  # every value of the six matrices written once; inputs are intermediate tables
        kernels.append(hbm_entry(
            "face_kernel", "k_face_pipe<3> (rows of the per-node response tables -> CSR values of the six matrices; "
            "software-pipelined persistent kernel)", face_bytes, face_ms, 1,
            "achieved = 8 B x nnz of the six output matrices / time (SURVEY 8(d) B_out values); the kernel also reads "
            "the response tables (node_table_doubles x 8 B, once if L2 / Infinity Cache hold the re-reads)", "face",
            {"table_bytes_read_once": 8.0 * st["node_table_doubles"]}))
        node_ms = ctx.time_kernel(1, reps=3)
        fp64_peak = 78.6e12  # MI355X vector FP64; FP64 MFMA has no higher rate on this part
        nnodes = st["num_nodes"]
        ref_flops = 1.2e6 * nnodes * (st["sum_block_sq"] / max(nnodes, 1) / 36.0 ** 2) ** 1.5  # ~1.2 MFLOP per 36-sub-face node
        # bound "mfma" = the compute roofline of the dtype: on MI355X the dense FP64 MFMA peak IS the vector FP64 peak
        # (78.6 TFLOP/s, MI355X_MICROARCH.md); the kernel issues vector FMAs (see "note")
        node_entry = {"bound": "mfma", "compute_unit": "FP64 vector FMA (FP64 MFMA has the same peak on this part)", "name": "node_kernel",
                      "kernel": "launch_node_class_reg<64,3,40> (interaction regions: nK, D^-1, condensed system, register "
                                "Gauss-Jordan with partial pivoting, response table A^-1 G)",
                      "achieved": st["node_flops"] / (node_ms * 1e-3) / 1e12, "peak": fp64_peak / 1e12, "unit": "TFLOP/s",
                      "frac": st["node_flops"] / (node_ms * 1e-3) / fp64_peak,
                      "flops_per_launch_executed": st["node_flops"],
                      "flops_per_launch_reference_formulation": ref_flops,
                      "frac_on_reference_formulation_flops": ref_flops / (node_ms * 1e-3) / fp64_peak,
                      "bytes_written_per_launch": 8.0 * st["node_table_doubles"],
                      "written_GBs": 8.0 * st["node_table_doubles"] / (node_ms * 1e-3) / 1e9,
                      "ms_per_launch": node_ms, "launches_per_step": 1, "ms_per_step": node_ms,
                      "traffic": (pmc.get("node", {}) or {}).get("traffic_bytes_per_launch"),
                      "note": "executed flops: the condensed n x n systems (n = 36 at an interior node of a tetrahedral grid) "
                              "are 8x less arithmetic than the reference's (nd deg)^2 gradient systems whose count SURVEY 8(d) "
                              "states; both fractions are given.  36 of 64 lanes hold a matrix row: the kernel is bound by "
                              "VALU issue (2 v_readlane + 1 v_fma_f64 per entry and pivot step), not by flops or bytes"}
        kernels.append(node_entry)
        kernels.sort(key=lambda e: -e["ms_per_step"])
        roofline = kernels[0]
        per_step_ms = {e["name"]: e["ms_per_step"] for e in kernels}

        # assembly phases (HBM-bound on their CSR output): algorithmic bytes = inputs once + outputs once
        # (the index array of vector_source -- nd x the flux pattern, a pure function of it -- is written on first use
        # and the timed step never asks for it: its 4 B x nnz are NOT counted, PFV_VS_INDICES_EAGER=1 restores both)
        vs_index_bytes = 4.0 * nnz["vs"] if os.environ.get("PFV_VS_INDICES_EAGER", "0") not in ("", "0") else 0.0
        out_bytes = 8.0 * sum(nnz.values()) + 4.0 * (nnz["flux"] + nnz["bound_flux"]) + vs_index_bytes + 12.0 * nnzA
        nfl, nnl = lp.raw["face_centers"].shape[1], lp.raw["nodes"].shape[1]
        in_bytes = 8.0 * (3 * nnl + 3 * nloc + 7 * nfl) + 72.0 * nloc + 5.0 * 4 * nloc + 4.0 * 3 * nfl
        # the interaction-region kernel runs beside the symbolic phase (second stream): the phases overlap, the
        # assembly time is the span of the discretize call plus div@flux / rhs
        asm_ms = st["discretize_ms"] + st["assemble_ms"]
        assembly = {"algorithmic_bytes": out_bytes + in_bytes, "ms": asm_ms,
                    "achieved_GBs": (out_bytes + in_bytes) / (asm_ms * 1e-3) / 1e9,
                    "frac_of_hbm_peak": (out_bytes + in_bytes) / (asm_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                    "frac_of_measured_triad": (out_bytes + in_bytes) / (asm_ms * 1e-3) / 1e9 / triad_gbs,
                    "phases_ms": {k: st[k] for k in ("topology_ms", "symbolic_ms", "node_ms", "face_ms",
                                                     "assemble_ms", "solve_ms", "discretize_ms")},
                    "phases_note": "symbolic_ms and node_ms are overlapping spans (two streams); discretize_ms is the whole call",
                    "cells_per_s_assembly_only": nloc / (asm_ms * 1e-3)}
        if world == 1 and not args.force_sharded:
            # the same grid with new parameter values (what a nonlinear model does every iteration): topology and
            # CSR patterns are kept, only the values are recomputed -- index bytes are then not part of the output
            ctx.discretize(rebuild_topology=False)
            ctx.sync()
            tw = time.perf_counter()
            for _ in range(3):
                ctx.discretize(rebuild_topology=False)
                ctx.assemble_device(d_bv.data_ptr(), 0, d_src.data_ptr())
            ctx.sync()
            warm_ms = 1e3 * (time.perf_counter() - tw) / 3
            warm_bytes = 8.0 * sum(nnz.values()) + 8.0 * nnzA + in_bytes
            assembly["values_only_rediscretization"] = {
                "ms": warm_ms, "algorithmic_bytes": warm_bytes, "achieved_GBs": warm_bytes / (warm_ms * 1e-3) / 1e9,
                "frac_of_hbm_peak": warm_bytes / (warm_ms * 1e-3) / 1e9 / HBM_PEAK_GBS,
                "note": "pfv_mpfa_discretize without PFV_DISCR_REBUILD_TOPOLOGY + div@flux: interaction-region kernel, face "
                        "kernel, system matrix; not the headline (the timed step rebuilds everything)"}
            # ... and the whole step of such an iteration: values-only discretization, assembly, and a solve whose AMG
            # setup keeps the aggregates of the previous matrix (only the Galerkin products are redone)
            d_xw = torch.zeros(nloc, dtype=torch.float64, device=dev)

            def warm_step():
                ctx.discretize(rebuild_topology=False)
                ctx.assemble_device(d_bv.data_ptr(), 0, d_src.data_ptr())
                return ctx.solve_device(d_xw.data_ptr(), "bicgstab", rtol=args.rtol, maxit=20000, raise_on_fail=False,
                                        precond=args.precond)

            warm_step()
            ctx.sync()
            tw = time.perf_counter()
            for _ in range(3):
                winfo = warm_step()
            ctx.sync()
            wstep_ms = 1e3 * (time.perf_counter() - tw) / 3
            stw = ctx.stats()
            assembly["values_only_step"] = {
                "ms_per_step": wstep_ms, "cells_per_s": nloc / (wstep_ms * 1e-3), "iterations": winfo["iterations"],
                "rel_residual": winfo["rel_residual"], "amg_setup_ms": stw["amg_setup_ms"], "amg_maps_reused": int(stw["amg_maps_reused"]),
                "rel_l2_vs_timed_solution": float(torch.linalg.norm(d_xw - x) / torch.linalg.norm(x)),
                "note": "secondary figure, not the headline: the step of a nonlinear iteration on a fixed grid (patterns, "
                        "topology and AMG aggregates kept; all values, the Galerkin products and the solve redone)"}

        if rank == 0 and world == 1 and not args.force_sharded:
            # field-level check of the timed configuration: the same system solved again (untimed) to the limit of
            # the arithmetic; the difference of the two solutions bounds the algebraic error of the timed one
            try:
                d_x2 = torch.zeros(nloc, dtype=torch.float64, device=dev)
                info2 = ctx.solve_device(d_x2.data_ptr(), "bicgstab", rtol=2e-15, maxit=400, raise_on_fail=False,
                                         precond=args.precond)
                xa, xb = x.cpu().numpy(), d_x2.cpu().numpy()
                field = {"rel_l2_change_vs_solve_to_2e-15": float(np.linalg.norm(xa - xb) / np.linalg.norm(xb)),
                         "max_abs_change": float(np.max(np.abs(xa - xb))), "max_abs_field": float(np.max(np.abs(xb))),
                         "tight_solve_true_rel_residual": info2["rel_residual"], "tight_solve_iterations": info2["iterations"]}
            except Exception as e:  # diagnostics only
                field = {"error": repr(e)}
        if rank == 0 and world == 1 and not args.no_cpu_baseline:
            cpu = cpu_baseline(args.cpu_n_side, args.cpu_port_n_side)
        if rank == 0 and world == 1 and args.cpu_headline > 0:
            cpu_headline = cpu_baseline_reference(args.n_side, timeout_s=3000.0, num_sub=args.cpu_headline, solve_cap_s=600.0)
        elif rank == 0 and world == 1 and args.n_side == 69:
            cpu_headline = cached_cpu_headline()
        if rank == 0 and world == 1 and not args.force_sharded and args.n_side == 69 and not args.no_whole_grid_check:
            try:
                whole_grid = whole_grid_check(pa, local_rank, args.rtol, args.precond)
                whole_grid.pop("_pattern", None)
            except Exception as e:  # diagnostics only
                whole_grid = {"error": repr(e)}
        if rank == 0 and world == 1 and not args.force_sharded and args.n_side == 69 and not args.no_extra_configs:
            try:
                opapi = bench_operator_api(pa, lp, Kvals, flags, bv, src, eta, local_rank)
            except Exception as e:  # secondary line only
                opapi = {"error": repr(e)}
            try:
                c2 = bench_config_c2(pa, local_rank, args.rtol, args.precond)
            except Exception as e:  # secondary line only
                c2 = {"error": repr(e)}
            try:
                c4 = bench_config_c4(pa, local_rank, args.rtol, args.precond)
            except Exception as e:  # secondary line only
                c4 = {"error": repr(e)}

        # ---- every rank's view of the run (N > 1; VERDICT r5 item 8: the first run on several GPUs must yield a diagnosable
        # curve, not one number): phases of the last timed step by the library's own HIP events, the step times by this rank's
        # clock, sizes, what the process group looks like from here, what travelled.  One all_gather_object after the clock stopped.
        if dist is not None:
            try:
                mine = {
                    "rank": rank, "local_rank": local_rank,
                    "device": torch.cuda.get_device_name(local_rank) if torch.cuda.is_available() else "cpu",
                    "ranks_seen_by_rccl": int(dist.get_world_size()), "backend": str(dist.get_backend()),
                    "cells_owned": int(nc), "cells_with_halo": int(nloc), "halo_fraction": float(nloc - nc) / max(float(nloc), 1.0),
                    "phases_ms": {k: float(st[k]) for k in ("topology_ms", "symbolic_ms", "node_ms", "face_ms", "assemble_ms",
                                                            "solve_ms", "discretize_ms", "amg_setup_ms") if k in st},
                    "kept": {"csr_patterns": int(st.get("symbolic_reused", 0)), "spmv_windows": int(st.get("win_reused", 0)),
                             "amg_aggregate_maps": int(st.get("amg_maps_reused", 0))},
                    "amg": {"levels": int(st.get("amg_levels", 0)), "coarsest_rows": int(st.get("amg_coarsest_rows", 0)),
                            "operator_complexity": float(st.get("amg_operator_complexity", 0.0))},
                    "launches": {"krylov_loop": int(st.get("solve_launches", 0)), "amg_setup": int(st.get("amg_setup_launches", 0))},
                    "step_ms_by_this_ranks_clock": [round(t, 2) for t, _ in each[:32]],
                    "iterations": [i for _, i in each[:32]],
                    "transport": (info.get("transport") if isinstance(info, dict) else None),
                    "halo_bytes_per_exchange": (info.get("halo_bytes_per_exchange") if isinstance(info, dict) else None),
                    "overlap_interior_boundary": os.environ.get("PFV_SHARD_OVERLAP", "0"),
                }
                per_rank = [None] * world
                dist.all_gather_object(per_rank, mine)
            except Exception as e:  # (diagnostics only: never costs the line)
                per_rank = [{"error": repr(e)}]

    if rank == 0:
        res_true = None
        try:
            if args.full and world == 1 and not args.force_sharded:
                b = ctx.rhs()
                xh = x if isinstance(x, np.ndarray) else x.cpu().numpy()
                res_true = float(np.linalg.norm(b - ctx.spmv(pa._lib.MAT_SYSTEM, xh)) / np.linalg.norm(b))
        except Exception:
            pass
        line = {
            "metric": "cells/sec MPFA assemble+solve, 3D unstructured grid",
            "value": value, "unit": "cells/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": args.scaling, "vs_baseline": None,
            "dtype": "f64", "data": "synthetic", "prewarm_steps_untimed": prewarm, "full": args.full,
            "config": {"workload": f"BASELINE configs[2] (the 2 M-cell grid the north_star target is quoted on): "
                                   f"3D simplex box, {nc} owned tetrahedra per GPU (n_side={args.n_side}), perturbed "
                                   "nodes, full-tensor anisotropic heterogeneous K, Dirichlet x-faces; every step: sub-cell "
                                   "topology + CSR patterns + MPFA-O discretization (6 matrices) + div@flux + AMG setup + "
                                   "preconditioned BiCGStab to rtol on the TRUE residual",
                       "cells_per_gpu": nc, "krylov": "bicgstab+" + args.precond, "rtol": args.rtol,
                       "amg": ({"levels": st["amg_levels"], "operator_complexity": st["amg_operator_complexity"],
                                "setup_ms": st["amg_setup_ms"], "coarsest_rows": st["amg_coarsest_rows"],
                                "filter_theta": st.get("amg_filter_theta"), "level0_entries": st.get("amg_level0_nnz")}
                               if args.precond in ("amg", "amg_block") else None),
                       "sharded_hierarchy": (None if sh is None else
                                             {"amg": "coupled (halo exchange on every level, coarse levels gathered and "
                                                     "replicated: pfv_amg_setup_sharded)",
                                              "amg_block": "block Jacobi across ranks (pfv_amg_setup(n_own))"}.get(args.precond)),
                       "solve_on_renumbered_copy": bool(st.get("solve_renumbered", 0)),
                       "ranks_seen_by_rccl": (dist.get_world_size() if dist is not None else 1),
                       "process_group_backend": (dist.get_backend() if dist is not None else None),
                       "self_launched": os.environ.get("PFV_BENCH_SELF_LAUNCHED") == "1",
                       "pattern_reuse": {"amg_aggregate_maps_kept": int(st.get("amg_maps_reused", 0)),
                                         "spmv_windows_kept": int(st.get("win_reused", 0)),
                                         "csr_patterns_kept": int(st.get("symbolic_reused", 0)),
                                         "symbolic_ms": st.get("symbolic_ms"),
                                         "amg_filter_layout": int(st.get("amg_filter_layout", 0)),
                                         "value_dependent_note": "amg_filter_layout 1 = the strength filter of the AMG setup wrote "
                                                                 "into the row layout of the previous step's filtering instead of "
                                                                 "counting + scanning first: only offered after a setup that "
                                                                 "reproduced the layout before it, so with a field that moves "
                                                                 "every step (the default) it stays 0; the filtered windows and the "
                                                                 "Galerkin sizes are kept only on an equal digest of the FILTERED "
                                                                 "index arrays, which moving values do not reproduce either",
                                         "note": "every step rebuilds the sub-cell topology, all values, the strength filter, the "
                                                 "Galerkin products and the solve, on a permeability field that changes from step "
                                                 "to step.  Kept when the REBUILT topology is proved equal (sizes + 64-bit digest "
                                                 "of every array the symbolic phase reads) to the one they were built from: the "
                                                 "CSR patterns of the six matrices and of A, the column maps and face records "
                                                 "(csr_patterns_kept; symbolic_ms then is the time of the proof; VERDICT r5 item 6); "
                                                 "kept on an equal digest of A's index arrays: the SpMV windows of A "
                                                 "(a function of the pattern alone) and the pairwise aggregate maps of the AMG "
                                                 "levels -- the latter follow the strength of connection of the VALUES they were "
                                                 "built from, i.e. the cycle coarsens along the previous step's field (what a "
                                                 "nonlinear iteration does); what that costs or saves shows against "
                                                 "ms_per_step_cold, where nothing is kept"},
                       "sparsity_pattern": "structural stencil: a superset of the reference's stored pattern (bit-identical on "
                                           "generic anisotropic inputs; where the reference's sparse products drop exact zeros, "
                                           "what is stored outside its pattern is < 1e-12 of the row maximum)",
                       "iterations": info["iterations"], "converged": info["converged"],
                       "true_rel_residual": res_true,
                       # (N > 1: the residual the sharded loop stopped on -- |b - A x| over all ranks by the recursion,
                       # re-evaluated from the definition every check interval; no rank holds the whole system)
                       "rel_residual_of_the_sharded_loop": (float(info["rel_residual"]) if sh is not None and isinstance(info, dict)
                                                            and info.get("rel_residual") is not None else None),
                       "field_error": field,
                       "global_cells": ncells_total,
                       "transport": (info.get("transport") if isinstance(info, dict) else None),
                       "parallelism": "1 GPU" if world == 1 else
                       f"{world} subdomains ({'x'.join(str(p) for p in (blocks or (1, 1, world)))} blocks of the box, 1 lattice "
                       "layer of halo cells recomputed per cut), assembly "
                       "without collectives, BiCGStab with RCCL point-to-point halo exchange + fused all-reduces; "
                       "AMG: per level and visit 2 point-to-point halo exchanges, one all-gather at the gathered level"},
            "each_timed_step": {"ms": [round(t, 2) for t, _ in each[:64]], "iterations": [i for _, i in each[:64]],
                                "note": "rank 0; the permeability field differs from step to step, and so do the iteration "
                                        "count and the sizes of everything the strength filter produces"},
            "permeability_per_step": ("one field repeated (--fixed-k)" if args.fixed_k else
                                      f"a new log-normal field every step ({n_fields} fields resident in HBM, cycled)"),
            "launches_per_iteration": (st.get("solve_launches", 0) / max(its, 1)) if its else None,
            "solve_launches": {"krylov_loop": int(st.get("solve_launches", 0)), "amg_setup": int(st.get("amg_setup_launches", 0)),
                               "note": "this library's kernel dispatches of the last timed solve (rocPRIM primitives, memsets and copies not counted)"},
        }
        if args.full:
            line.update({
                "roofline": roofline, "roofline_kernels": kernels[1:], "kernel_ms_per_step": per_step_ms,
                "hbm_triad_measured_GBs": triad_gbs, "hbm_read_stream_measured_GBs": read_gbs,
                "ms_per_step_cold": (cold or {}).get("ms_per_step_cold"), "cold_step": cold,
                "whole_grid_check": whole_grid,
                "per_rank": per_rank,
                "assembly": assembly, "operator_api": opapi, "cpu_baseline": cpu, "cpu_baseline_headline_grid": cpu_headline,
                "config_c2": c2, "config_c4": c4,
                "config_c5": (config_c5(args.c5) if (world == 1 and args.n_side == 69 and (args.c5 or not args.no_extra_configs)) else None),
            })
        if args.phases:
            print(json.dumps(st, indent=1), file=sys.stderr)
        record_out.write(json.dumps(line) + "\n")
        record_out.flush()
    if dist is not None:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
