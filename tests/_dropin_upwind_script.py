"""Run inside a subprocess with the REFERENCE PorePy importable: ``pp.Upwind`` against the class
``porepy_amd.as_porepy_upwind()`` returns, on the reference's own grids and parameter dictionaries."""
import json

import numpy as np
import scipy.sparse as sps

import porepy as pp

import porepy_amd as pa
from tests import _parity as P


def same(a, b):
    a, b = sps.csr_matrix(a), sps.csr_matrix(b)
    a.sort_indices()
    b.sort_indices()
    return bool(a.shape == b.shape and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
                and a.data.tobytes() == b.data.astype(np.float64).tobytes())


def case(g, q, bc, bv, Hip, flux_key=None, k=1):
    res = {}
    outs = []
    for cls in (pp.Upwind, Hip):
        par = {"bc_values": bv, (flux_key or "darcy_flux"): q}
        if bc is not None:
            par["bc"] = bc
        if k != 1:
            par["num_components"] = k
        data = pp.initialize_data({}, "transport", par)
        up = cls("transport")
        if flux_key:
            up.flux_array_key = flux_key
        up.discretize(g, data)
        md = data[pp.DISCRETIZATION_MATRICES]["transport"]
        A, b = up.assemble_matrix_rhs(g, data) if k == 1 else (None, None)
        outs.append((md, A, b, up))
    (m0, A0, b0, _), (m1, A1, b1, hip) = outs
    res["is_subclass"] = isinstance(hip, pp.Upwind)
    res["matrices_identical"] = all(same(m0[key], m1[key]) for key in ("transport", "rhs_dir", "rhs_neu"))
    if k == 1:
        d = abs(sps.csr_matrix(A1) - sps.csr_matrix(A0))
        res["A_rel_err"] = float((d.max() if d.nnz else 0.0) / abs(A0).max())
        res["rhs_rel_err"] = float(np.abs(b1 - b0).max() / max(np.abs(b0).max(), 1e-300))
    res["flux_helper_err"] = float(np.abs(hip._hip.darcy_flux(g, [0.3, -0.2, 0.1]) - pp.Upwind("t").darcy_flux(g, [0.3, -0.2, 0.1])).max())
    ap = 0.5 + np.arange(g.num_cells) / g.num_cells
    res["flux_helper_aperture_err"] = float(np.abs(hip._hip.darcy_flux(g, [0.3, -0.2, 0.1], ap)
                                                   - pp.Upwind("t").darcy_flux(g, [0.3, -0.2, 0.1], ap)).max())
    return res


def main():
    lib = P.dropin_library()
    Hip = pa.as_porepy_upwind(library=lib)
    rng = np.random.default_rng(4)
    out = {}
    g = pp.CartGrid([4, 3], [4.0, 3.0])
    g.compute_geometry()
    bf = g.get_all_boundary_faces()
    bc = pp.BoundaryCondition(g, bf, list(np.array(["dir", "neu"])[np.arange(bf.size) % 2]))
    bv = np.zeros(g.num_faces)
    bv[bf] = rng.random(bf.size)
    q = rng.random(g.num_faces) - 0.5
    out["cart2d"] = case(g, q, bc, bv, Hip)
    out["cart2d_custom_flux_key"] = case(g, q, bc, bv, Hip, flux_key="my_flux")
    out["cart2d_two_components"] = case(g, q, bc, bv, Hip, k=2)
    g3 = pp.StructuredTetrahedralGrid([3, 3, 3], [1, 1, 1])
    g3.compute_geometry()
    bv3 = np.zeros(g3.num_faces)
    bf3 = g3.get_all_boundary_faces()
    bv3[bf3] = rng.random(bf3.size)
    out["tet3d_default_bc"] = case(g3, pp.Upwind("t").darcy_flux(g3, [0.5, 0.2, -0.4]), None, bv3, Hip)
    g1 = pp.CartGrid([8], [2.0])
    g1.compute_geometry()
    out["line1d"] = case(g1, -np.ones(g1.num_faces), None, np.ones(g1.num_faces), Hip)
    out["library"] = str(lib._name)
    print("RESULT " + json.dumps(out))


if __name__ == "__main__":
    main()
