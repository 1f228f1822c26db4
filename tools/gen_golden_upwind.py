"""Golden fixtures for the upwind discretization, made by running the REFERENCE
(numerics/fv/upwind.py:67-335) -> tests/golden/upwind/upwind_*.npz (arrays only).

TEST INFRASTRUCTURE; needs the reference next to the repository:

    PYTHONDONTWRITEBYTECODE=1 PYTHONPATH=<repo>/oracle/shim:<reference>/src:<repo> python tools/gen_golden_upwind.py

The fixtures live in a sub-directory of their own: tests/_golden.py reads every file directly under
tests/golden/ with an unknown prefix as an MPFA case.
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

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "upwind")
KW = "transport"


def save(name, g, q, bc, bc_values, num_components=1, extra=None):
    params = {"darcy_flux": q, "bc_values": bc_values}
    if bc is not None:
        params["bc"] = bc
    if num_components != 1:
        params["num_components"] = num_components
    data = pp.initialize_data({}, KW, params)
    up = pp.Upwind(KW)
    up.discretize(g, data)
    md = data[pp.DISCRETIZATION_MATRICES][KW]
    store = {}
    for k, v in grid_to_raw(g).items():
        store["grid_" + k] = np.asarray(v)
    store["has_bc"] = np.array(bc is not None)
    if bc is not None:
        for k, v in bc_to_raw(bc).items():
            store["bc_" + k] = v
    store["flux"] = np.asarray(q, dtype=np.float64)
    store["bc_values"] = np.asarray(bc_values, dtype=np.float64)
    store["num_components"] = np.array(num_components)
    for key in ("transport", "rhs_dir", "rhs_neu"):
        pack_csr("ref_" + key, md[key], store)
    nnz = [md[k].nnz for k in ("transport", "rhs_dir", "rhs_neu")]
    if num_components == 1 and g.dim > 0:
        A, rhs = up.assemble_matrix_rhs(g, data)
        pack_csr("ref_A", A, store)
        store["ref_rhs"] = np.asarray(rhs, dtype=np.float64)
        nnz.append(sps.csr_matrix(A).nnz)
    if extra:
        store.update(extra)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **store)
    print(f"{name:28s} cells={g.num_cells:4d} faces={g.num_faces:4d} nnz={nnz} {os.path.getsize(path) / 1024:.0f} KiB")


def mixed(g, kinds):
    bf = g.get_all_boundary_faces()
    return pp.BoundaryCondition(g, bf, list(np.array(kinds)[np.arange(bf.size) % len(kinds)]))


def bvals(g, rng):
    v = np.zeros(g.num_faces)
    bf = g.get_all_boundary_faces()
    v[bf] = rng.random(bf.size) + 0.25
    return v


def main():
    os.makedirs(OUT, exist_ok=True)
    rng = np.random.default_rng(20261016)
    up = pp.Upwind(KW)

    # 1. 1-D line, 8 cells, dir / neu ends, both flux directions
    for sgn, tag in ((1.0, "pos"), (-1.0, "neg")):
        g = pp.CartGrid([8], [2.0]); g.compute_geometry()
        bf = g.get_all_boundary_faces()
        bc = pp.BoundaryCondition(g, bf, ["dir", "neu"])
        save(f"upwind_line8_{tag}", g, up.darcy_flux(g, [sgn * 1.5, 0, 0]), bc, bvals(g, rng))

    # 2. Cartesian 4x3, x-aligned constant field: 16 of 31 faces carry zero flux
    g = pp.CartGrid([4, 3], [4.0, 3.0]); g.compute_geometry()
    q = up.darcy_flux(g, [1.0, 0, 0])
    assert (q == 0).sum() == 16
    bf = g.get_all_boundary_faces()
    save("upwind_cart4x3_xfield", g, q, pp.BoundaryCondition(g, bf, ["dir"] * bf.size), bvals(g, rng))

    # 3. same grid: -0.0, a tiny negative, sign changes; mixed dir / neu
    q = (rng.random(g.num_faces) - 0.5) * 2.0
    q[3] = -0.0
    q[7] = -1e-300
    q[11] = 0.0
    q[20] = -0.0
    q[25] = -1e-300
    save("upwind_cart4x3_signs", g, q, mixed(g, ["dir", "neu"]), bvals(g, rng))

    # 4. perturbed triangles, rotating field; mixed dir / neu, and no "bc" key at all
    g = perturb_interior(pp.StructuredTriangleGrid([5, 4], [1.0, 1.0]), rng, 0.05)
    fc = g.face_centers
    vel = np.vstack([-(fc[1] - 0.5), fc[0] - 0.5, np.zeros(g.num_faces)])
    q = np.sum(vel * g.face_normals, axis=0)
    save("upwind_tri5x4_rot", g, q, mixed(g, ["dir", "dir", "neu"]), bvals(g, rng))
    save("upwind_tri5x4_rot_nobc", g, q, None, bvals(g, rng))

    # 5. perturbed 3x3x3 tetrahedra: q from the reference's own MPFA solve (heterogeneous full tensor)
    g = perturb_interior(pp.StructuredTetrahedralGrid([3, 3, 3], [1, 1, 1]), rng, 0.06)
    nc = g.num_cells
    k = 1 + rng.random(nc)
    K = pp.SecondOrderTensor(kxx=k, kyy=2 * k, kzz=0.5 * k, kxy=0.2 * k, kxz=0.05 * k, kyz=0.1 * k)
    fbc = mixed(g, ["dir", "dir", "neu"])
    fbv = np.zeros(g.num_faces)
    bf = g.get_all_boundary_faces()
    fbv[bf] = np.where(fbc.is_dir[bf], g.face_centers[:, bf].sum(axis=0), 0.1 * (rng.random(bf.size) - 0.5))
    fdata = pp.initialize_data({}, "flow", {"second_order_tensor": K, "bc": fbc, "bc_values": fbv,
                                            "mpfa_inverter": "python"})
    mp = pp.Mpfa("flow")
    mp.discretize(g, fdata)
    A, b = mp.assemble_matrix_rhs(g, fdata)
    import scipy.sparse.linalg as spla

    p = spla.spsolve(sps.csc_matrix(A), b)
    fm = fdata[pp.DISCRETIZATION_MATRICES]["flow"]
    q = fm["flux"] @ p + fm["bound_flux"] @ fbv
    extra = {"flow_perm": np.ascontiguousarray(K.values), "flow_bc_values": fbv, "flow_p": p}
    for kk, v in bc_to_raw(fbc).items():
        extra["flowbc_" + kk] = v
    save("upwind_tet3x3x3_mpfa", g, q, mixed(g, ["dir", "neu"]), bvals(g, rng), extra=extra)

    # 6. two components (discretization matrices only)
    g = pp.CartGrid([4, 3], [4.0, 3.0]); g.compute_geometry()
    q = (rng.random(g.num_faces) - 0.5)
    save("upwind_cart4x3_k2", g, q, mixed(g, ["neu", "dir"]), np.zeros(g.num_faces), num_components=2)

    # 7. a 2-D grid tilted in 3-D, and a 0-D grid's shapes
    g = pp.CartGrid([3, 3], [1.0, 1.0])
    c, s = np.cos(0.7), np.sin(0.7)
    R = np.array([[1, 0, 0], [0, c, -s], [0, s, c]]) @ np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    g.nodes = R @ g.nodes
    g.compute_geometry()
    q = up.darcy_flux(g, R @ np.array([0.7, -0.4, 0.0]))
    save("upwind_tilted3x3", g, q, mixed(g, ["dir", "neu"]), bvals(g, rng))
    g0 = pp.PointGrid(np.zeros(3)); g0.compute_geometry()
    data = pp.initialize_data({}, KW, {"darcy_flux": np.zeros(0)})
    up.discretize(g0, data)
    md = data[pp.DISCRETIZATION_MATRICES][KW]
    np.savez_compressed(os.path.join(OUT, "upwind_point0d.npz"),
                        shapes=np.array([md["transport"].shape, md["rhs_dir"].shape, md["rhs_neu"].shape], dtype=np.int64))
    print("upwind_point0d shapes", md["transport"].shape, md["rhs_dir"].shape, md["rhs_neu"].shape)


if __name__ == "__main__":
    main()
