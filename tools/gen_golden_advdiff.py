"""Golden fixtures for the advection-diffusion system, made by running the REFERENCE's pp.Mpfa / pp.Tpfa and
pp.Upwind on ONE parameter dictionary -> tests/golden/advdiff/advdiff_*.npz (arrays only).

TEST INFRASTRUCTURE; needs the reference next to the repository:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<repo>/oracle/shim:<reference>/src:<repo> python tools/gen_golden_advdiff.py

Per case: the raw grid, the tensor, the bc flags, bc_values, q, flux_scale w; the reference's (A_D, b_D) of the
diffusion, (A_U, b_U) of the upwind term for q, and b_Uw for the flux w q (equal to b_U when w = 1: the Dirichlet
inflow carries the scaled flux, a Neumann value is a flux already); an acc, a c0 and a source for the stepping tests.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import scipy.sparse as sps

import porepy as pp

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle.gen_golden import pack_csr, perturb_interior  # noqa: E402
from oracle.ref_bridge import bc_to_raw, grid_to_raw  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "advdiff")
KW = "transport"


def mixed(g, kinds):
    bf = g.get_all_boundary_faces()
    return pp.BoundaryCondition(g, bf, list(np.array(kinds)[np.arange(bf.size) % len(kinds)]))


def save(name, g, K, bc, bc_values, q, rng, scheme="mpfa", w=1.0):
    params = {"second_order_tensor": K, "bc": bc, "bc_values": bc_values, "darcy_flux": q, "mpfa_inverter": "python"}
    data = pp.initialize_data({}, KW, params)
    diff = (pp.Mpfa if scheme == "mpfa" else pp.Tpfa)(KW)
    diff.discretize(g, data)
    A_D, b_D = diff.assemble_matrix_rhs(g, data)
    up = pp.Upwind(KW)
    up.discretize(g, data)
    A_U, b_U = up.assemble_matrix_rhs(g, data)
    data_w = pp.initialize_data({}, KW, dict(params, darcy_flux=w * q))
    up.discretize(g, data_w)
    _, b_Uw = up.assemble_matrix_rhs(g, data_w)
    store = {}
    for k, v in grid_to_raw(g).items():
        store["grid_" + k] = np.asarray(v)
    for k, v in bc_to_raw(bc).items():
        store["bc_" + k] = v
    store["perm"] = np.ascontiguousarray(K.values)
    store["bc_values"] = np.asarray(bc_values, dtype=np.float64)
    store["flux"] = np.asarray(q, dtype=np.float64)
    store["flux_scale"] = np.array(float(w))
    store["tpfa"] = np.array(scheme == "tpfa")
    pack_csr("ref_AD", sps.csr_matrix(A_D), store)
    pack_csr("ref_AU", sps.csr_matrix(A_U), store)
    store["ref_bD"] = np.asarray(b_D, dtype=np.float64)
    store["ref_bU"] = np.asarray(b_U, dtype=np.float64)
    store["ref_bUw"] = np.asarray(b_Uw, dtype=np.float64)
    store["acc"] = (0.2 + 0.3 * rng.random(g.num_cells)) * g.cell_volumes / 0.05
    store["c0"] = rng.random(g.num_cells)
    store["source"] = 0.1 * (rng.random(g.num_cells) - 0.5) * g.cell_volumes
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **store)
    print(f"{name:28s} {scheme} cells={g.num_cells:4d} faces={g.num_faces:4d} nnz(A_D)={sps.csr_matrix(A_D).nnz} "
          f"nnz(A_U)={sps.csr_matrix(A_U).nnz} {os.path.getsize(path) / 1024:.0f} KiB")


def bvals(g, rng):
    v = np.zeros(g.num_faces)
    bf = g.get_all_boundary_faces()
    v[bf] = rng.random(bf.size) + 0.25
    return v


def signed_flux(g, rng):
    """Both signs, exact zeros (+0 and -0) on interior faces, outflow and inflow on the Dirichlet faces."""
    q = rng.standard_normal(g.num_faces)
    interior = np.setdiff1d(np.arange(g.num_faces), g.get_all_boundary_faces())
    pick = rng.choice(interior, size=max(2, interior.size // 8), replace=False)
    q[pick[::2]] = 0.0
    q[pick[1::2]] = -0.0
    return q


def aniso(g, rng):
    k = 1 + rng.random(g.num_cells)
    if g.dim == 3:
        return pp.SecondOrderTensor(kxx=k, kyy=2 * k, kzz=0.5 * k, kxy=0.2 * k, kxz=0.05 * k, kyz=0.1 * k)
    return pp.SecondOrderTensor(kxx=k, kyy=1.5 * k, kxy=0.3 * k)


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261017)
    up = pp.Upwind(KW)

    # 1. Cartesian 4x5, mixed conditions, signed flux with zeros; MPFA and TPFA
    g = pp.CartGrid([4, 5], [4.0, 5.0]); g.compute_geometry()
    q = signed_flux(g, rng)
    save("advdiff_cart4x5_mpfa", g, aniso(g, rng), mixed(g, ["dir", "neu"]), bvals(g, rng), q, rng)
    save("advdiff_cart4x5_tpfa", g, pp.SecondOrderTensor(1 + rng.random(g.num_cells)), mixed(g, ["dir", "dir", "neu"]),
         bvals(g, rng), q, rng, scheme="tpfa")

    # 2. perturbed triangles, rotating field
    g = perturb_interior(pp.StructuredTriangleGrid([5, 4], [1.0, 1.0]), rng, 0.05)
    fc = g.face_centers
    vel = np.vstack([-(fc[1] - 0.5), fc[0] - 0.5, np.zeros(g.num_faces)])
    q = np.sum(vel * g.face_normals, axis=0)
    save("advdiff_tri5x4_rot", g, aniso(g, rng), mixed(g, ["dir", "dir", "neu"]), bvals(g, rng), q, rng)

    # 3. perturbed tetrahedra 3^3 and 4^3, anisotropic heterogeneous tensor; the second with flux_scale != 1
    g = perturb_interior(pp.StructuredTetrahedralGrid([3, 3, 3], [1, 1, 1]), rng, 0.06)
    save("advdiff_tet3_signed", g, aniso(g, rng), mixed(g, ["dir", "neu"]), bvals(g, rng), signed_flux(g, rng), rng)
    g = perturb_interior(pp.StructuredTetrahedralGrid([4, 4, 4], [1, 1, 1]), rng, 0.04)
    q = up.darcy_flux(g, [0.6, -0.3, 0.45])
    save("advdiff_tet4_scaled", g, aniso(g, rng), mixed(g, ["dir", "dir", "neu"]), bvals(g, rng), q, rng, w=4.18)
    g = perturb_interior(pp.StructuredTetrahedralGrid([3, 3, 3], [1, 1, 1]), rng, 0.06)
    save("advdiff_tet3_tpfa", g, pp.SecondOrderTensor(1 + rng.random(g.num_cells)), mixed(g, ["dir", "neu"]),
         bvals(g, rng), signed_flux(g, rng), rng, scheme="tpfa")

    # 4. 1-D line (TPFA: what Mpfa hands 1-D grids to), dir / neu ends, both directions
    for sgn, tag in ((1.0, "pos"), (-1.0, "neg")):
        g = pp.CartGrid([8], [2.0]); g.compute_geometry()
        bf = g.get_all_boundary_faces()
        bc = pp.BoundaryCondition(g, bf, ["dir", "neu"])
        save(f"advdiff_line8_{tag}", g, pp.SecondOrderTensor(0.5 + rng.random(g.num_cells)), bc, bvals(g, rng),
             up.darcy_flux(g, [sgn * 1.5, 0, 0]), rng, scheme="tpfa")


if __name__ == "__main__":
    main()
